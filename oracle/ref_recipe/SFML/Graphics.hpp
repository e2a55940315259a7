/* A stand-in for <SFML/Graphics.hpp> (TEST INFRASTRUCTURE): just enough of SFML's public names for
 * the reference's preview-window code to compile.  Nothing here draws; the window is never open. */
#ifndef RT_REF_SFML_STANDIN_HPP
#define RT_REF_SFML_STANDIN_HPP
#include <string>
namespace sf {
typedef unsigned char Uint8;
struct VideoMode { VideoMode(unsigned int, unsigned int) {} };
struct Event { enum EventType { Closed }; EventType type; };
struct Texture { bool create(unsigned int, unsigned int) { return true; } void update(const Uint8 *) {} };
struct Sprite { explicit Sprite(const Texture &) {} };
struct RenderWindow {
    RenderWindow(VideoMode, const std::string &) {}
    bool isOpen() const { return false; }
    bool pollEvent(Event &) { return false; }
    void close() {}
    void draw(const Sprite &) {}
    void display() {}
};
}
#endif
