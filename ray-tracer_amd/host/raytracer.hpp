/*
 * raytracer.hpp — C++ host-side mirror of the reference's scene / camera / render interface,
 * header-only over the C ABI (include/rt_amd.h, libraytracer_amd.so).
 *
 * A reference scene transcribes 1:1: the class and factory names, argument order and error
 * behaviour are the reference's (file:line cited per item, relative to the reference
 * checkout); what happens behind them is not.  Differences a caller sees:
 *   - image size, camera pose, spp, bounce limit, scene and seed are run-time values, not
 *     compile-time constants (SURVEY.md §5 "config / flags");
 *   - no __constant__ globals: Camera, RenderData and the committed scene are passed to
 *     render();
 *   - errors from the device layer are std::runtime_error("Error from HIP (<what>): <detail>")
 *     (reference: "Error from CUDA (...)", src/utils.cu:5-10).
 */
#ifndef RAYTRACER_AMD_HPP
#define RAYTRACER_AMD_HPP

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rt_amd.h"

namespace rtamd {

/* src/utils.cu:13-163 (host subset) */
struct Vec3 {
    float x = 0, y = 0, z = 0;
    Vec3() {}
    Vec3(float vx, float vy, float vz) : x(vx), y(vy), z(vz) {}
    Vec3 operator+(Vec3 o) const { return Vec3(x + o.x, y + o.y, z + o.z); }
    Vec3 operator-(Vec3 o) const { return Vec3(x - o.x, y - o.y, z - o.z); }
    Vec3 operator*(float s) const { return Vec3(x * s, y * s, z * s); }
    Vec3 operator/(float s) const { return Vec3(x / s, y / s, z / s); }
    const float *data() const { return &x; }
};

/* src/utils.cu:166-185 */
struct Vec2 {
    float x = 0, y = 0;
    Vec2() {}
    Vec2(float vx, float vy) : x(vx), y(vy) {}
};

/* src/objects.cu:19-22 */
struct Vertex {
    Vec3 world_point;
    Vec2 texture_point;
};

/* src/material.cu:4-125 */
class Texture {
public:
    static const int COLOUR = 0, GRADIENT = 1, CHECKERBOARD = 2, IMAGE = 3;
    int type = COLOUR;
    Vec3 colour, light, dark;
    int num_squares = 0;

    static Texture create_const_colour(Vec3 texture_colour) { Texture t; t.type = COLOUR; t.colour = texture_colour; return t; }
    static Texture create_gradient() { Texture t; t.type = GRADIENT; return t; }
    static Texture create_checkerboard(Vec3 light_colour, Vec3 dark_colour, int num_sq)
    {
        Texture t; t.type = CHECKERBOARD; t.light = light_colour; t.dark = dark_colour; t.num_squares = num_sq; return t;
    }
    /* src/material.cu:41-51; the texels (row-major rgb floats) must stay alive until the material has
     * been added to a scene (the scene keeps its own copy) */
    static Texture create_image(int width, int height, const float *rgb)
    {
        Texture t; t.type = IMAGE; t.img_w = width; t.img_h = height; t.img_rgb = rgb; return t;
    }
    int img_w = 0, img_h = 0;
    const float *img_rgb = nullptr;
};

/* ImageTexture src/main.cu:40-91: one entry of the baked texture file textures/parse_textures.py writes */
class ImageTexture {
public:
    std::string PARSED_TEXTURE_FILENAME = "textures/parsed_textures.txt";

    explicit ImageTexture(const std::string &filename) { parse_file(filename); }
    ImageTexture(const std::string &filename, const std::string &parsed_texture_filename) : PARSED_TEXTURE_FILENAME(parsed_texture_filename) { parse_file(filename); }
    Texture get_device_texture() const { return Texture::create_image(width, height, rgb_values.data()); }

private:
    int width = 0, height = 0;
    std::vector<float> rgb_values;

    void parse_file(const std::string &filename)
    {
        int32_t w = 0, h = 0;
        float *rgb = nullptr;
        rt_status st = rt_image_texture_load(PARSED_TEXTURE_FILENAME.c_str(), filename.c_str(), &w, &h, &rgb);
        if (st == RT_ERR_IO) throw std::runtime_error("Could not find file to open.");       /* src/obj_read.cu:10 */
        if (st != RT_OK) throw std::runtime_error("Image file not found.\n");                /* src/main.cu:72 */
        width = w; height = h;
        rgb_values.assign(rgb, rgb + (size_t)w * (size_t)h * 3);
        rt_image_texture_free(rgb);
    }
};

/* src/material.cu:128-186 */
class Material {
public:
    static const int STANDARD = 0, EMISSIVE = 1, REFRACTIVE = 2;
    rt_material c{};

    static Material create_standard(Texture mat_tex, float smoothness_val)
    {
        Material m;
        switch (mat_tex.type) {
            case Texture::COLOUR: rt_material_standard(&m.c, mat_tex.colour.data(), smoothness_val); break;
            case Texture::GRADIENT: rt_material_gradient(&m.c, smoothness_val); break;
            case Texture::CHECKERBOARD: rt_material_checkerboard(&m.c, mat_tex.light.data(), mat_tex.dark.data(), mat_tex.num_squares, smoothness_val); break;
            case Texture::IMAGE: rt_material_image(&m.c, mat_tex.img_w, mat_tex.img_h, mat_tex.img_rgb, smoothness_val); break;
            default: throw std::logic_error("unknown texture type");
        }
        return m;
    }
    static Material create_emissive(Vec3 emit_colour, float emit_strength)
    {
        Material m;
        rt_material_emissive(&m.c, emit_colour.data(), emit_strength);
        return m;
    }
    static Material create_refractive(Texture mat_tex, float n)
    {
        Material m;
        rt_material_refractive(&m.c, mat_tex.colour.data(), n);
        return m;
    }
};

/* src/obj_read.cu:47-147 */
class ObjFileMesh {
public:
    explicit ObjFileMesh(const std::string &filename)
    {
        rt_status st = rt_obj_load(filename.c_str(), &h_);
        if (st == RT_ERR_IO) throw std::runtime_error("Could not find file to open.");   /* :10 */
        if (st != RT_OK) throw std::runtime_error("Could not parse " + filename);
    }
    ~ObjFileMesh() { rt_obj_destroy(h_); }
    ObjFileMesh(const ObjFileMesh &) = delete;
    ObjFileMesh &operator=(const ObjFileMesh &) = delete;
    ObjFileMesh(ObjFileMesh &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }

    void enlarge(float scale_fact) { rt_obj_enlarge(h_, scale_fact); }
    void rotate(float x_angle, float y_angle, float z_angle) { rt_obj_rotate(h_, x_angle, y_angle, z_angle); }
    void translate(float offset_x, float offset_y, float offset_z) { rt_obj_translate(h_, offset_x, offset_y, offset_z); }
    int num_vertices() const { return rt_obj_num_vertices(h_); }
    int num_faces() const { return rt_obj_num_faces(h_); }
    /* the mesh's triangles, nine floats each, in the order a scene commits them (a quad gives two): what Renderer::update_mesh takes */
    std::vector<float> triangles() const
    {
        const int n = rt_obj_num_triangles(h_);
        if (n < 0) throw std::logic_error("Only triangle or quad meshes are supported.\n");
        std::vector<float> out((size_t)n * 9);
        if (n > 0 && rt_obj_get_triangles(h_, out.data()) != RT_OK) throw std::invalid_argument("face references a missing vertex");
        return out;
    }
    const rt_obj *handle() const { return h_; }

private:
    rt_obj *h_ = nullptr;
};

/* The scene's object list: std::vector<Object> + Object::create_* (src/objects.cu:845-906,
 * src/main.cu:94-296).  Objects are appended in call order. */
class SceneObjects {
public:
    bool use_sky = true;

    SceneObjects()
    {
        if (rt_scene_builder_create(&b_) != RT_OK) throw std::bad_alloc();
    }
    /* SceneObjects(int test_scene) src/main.cu:100-122: scenes 0, 1 and 3 */
    SceneObjects(int test_scene, const std::string &models_dir) : SceneObjects()
    {
        switch (test_scene) {
            case 0: monkey_test_scene(models_dir); break;
            case 1: reflection_test_scene(); break;
            case 3: refract_test_scene(); break;
            case 2: texture_test_scene(); break;                                   /* needs textures/parsed_textures.txt (not shipped upstream), like the reference */
            case 4: throw std::logic_error("scene 4 is unseeded in the reference; use ray-tracer_amd.scenes.reference_scene4");
            default: throw std::domain_error("Test scene must be number between 0 and 3 (inclusive).\n");   /* :118 */
        }
    }
    ~SceneObjects() { rt_scene_builder_destroy(b_); }
    SceneObjects(const SceneObjects &) = delete;
    SceneObjects &operator=(const SceneObjects &) = delete;

    void create_sphere(Vec3 center, float radius, const Material &mat) { check(rt_scene_add_sphere(b_, center.data(), radius, &mat.c)); }
    void create_triangle(Vec3 p1, Vec3 p2, Vec3 p3, const Material &mat) { check(rt_scene_add_triangle(b_, p1.data(), p2.data(), p3.data(), &mat.c)); }
    void create_triangle(Vertex p1, Vertex p2, Vertex p3, const Material &mat)
    {
        const float p[9] = {p1.world_point.x, p1.world_point.y, p1.world_point.z, p2.world_point.x, p2.world_point.y, p2.world_point.z,
                            p3.world_point.x, p3.world_point.y, p3.world_point.z};
        const float uv[6] = {p1.texture_point.x, p1.texture_point.y, p2.texture_point.x, p2.texture_point.y, p3.texture_point.x, p3.texture_point.y};
        check(rt_scene_add_triangle_uv(b_, p, uv, &mat.c));
    }
    void create_quad(Vec3 p1, Vec3 p2, Vec3 p3, Vec3 p4, const Material &mat) { check(rt_scene_add_quad(b_, p1.data(), p2.data(), p3.data(), p4.data(), &mat.c)); }
    void create_one_way_quad(Vec3 p1, Vec3 p2, Vec3 p3, Vec3 p4, bool invert_normal, const Material &mat)
    {
        check(rt_scene_add_one_way_quad(b_, p1.data(), p2.data(), p3.data(), p4.data(), invert_normal ? 1 : 0, &mat.c));
    }
    void create_cuboid(Vec3 tl_near_pos, float width, float height, float depth, const Material &mat)
    {
        check(rt_scene_add_cuboid(b_, tl_near_pos.data(), width, height, depth, &mat.c));
    }
    /* SceneObjects::create_mesh src/main.cu:127-148 */
    void create_mesh(const ObjFileMesh &obj, const Material &mat) { check(rt_scene_add_obj_mesh(b_, obj.handle(), &mat.c)); }
    /* ... from an array of triangles, nine floats each (rt_scene_add_mesh) */
    void create_mesh(const std::vector<float> &triangles, const Material &mat)
    {
        if (triangles.size() % 9) throw std::invalid_argument("nine floats per triangle");
        check(rt_scene_add_mesh(b_, triangles.data(), (int32_t)(triangles.size() / 9), &mat.c));
    }

    /* create_cornell_box src/main.cu:252-288 */
    void create_cornell_box(Vec3 tl_near_pos, float width, float height, float depth, float light_width)
    {
        use_sky = false;
        Material floor = Material::create_standard(Texture::create_checkerboard(Vec3(0.1f, 0.8f, 0.1f), Vec3(0.1f, 0.5f, 0.1f), 8), 0);
        Material l_wall = Material::create_standard(Texture::create_const_colour(Vec3(1, 0.2f, 0.2f)), 0);
        Material r_wall = Material::create_standard(Texture::create_const_colour(Vec3(0.3f, 0.3f, 1)), 0);
        Material back = Material::create_standard(Texture::create_const_colour(Vec3(0.2f, 0.2f, 0.2f)), 0);
        Material roof = Material::create_standard(Texture::create_const_colour(Vec3(0.9f, 0.9f, 0.9f)), 0);
        Material front = Material::create_standard(Texture::create_const_colour(Vec3(1, 1, 1)), 0);
        Vec3 w(width, 0, 0), h(0, height, 0), d(0, 0, depth), p = tl_near_pos;
        create_quad(p - h, p - h + w, p - h + w + d, p - h + d, floor);
        create_quad(p, p - h, p - h + d, p + d, l_wall);
        create_quad(p + w, p + w - h, p + w - h + d, p + w + d, r_wall);
        create_quad(p + d, p + w + d, p + w - h + d, p - h + d, back);
        create_quad(p, p + d, p + w + d, p + w, roof);
        create_one_way_quad(p, p + w, p + w - h, p - h, false, front);
        Material light_mat = Material::create_emissive(Vec3(1, 1, 1), 6);
        Vec3 light_tl(p.x + width / 2 - light_width / 2, p.y, p.z + depth / 2 - light_width / 2);
        create_cuboid(light_tl, light_width, 0.04f, light_width, light_mat);
    }

    int num_objects() const { return rt_scene_builder_num_objects(b_); }
    const rt_scene_builder *handle() const { return b_; }

private:
    rt_scene_builder *b_ = nullptr;

    void check(rt_status st)
    {
        if (st == RT_OK) return;
        std::string msg = rt_scene_builder_error(b_);
        if (st == RT_ERR_UNSUPPORTED) throw std::logic_error(msg);      /* src/main.cu:141 */
        throw std::invalid_argument(msg);
    }
    void monkey_test_scene(const std::string &models_dir)
    {   /* src/main.cu:150-170 */
        create_cornell_box(Vec3(-0.5f, 0.5f, 1.2f), 1, 1, 1, 0.5f);
        ObjFileMesh m(models_dir + "/low_poly_monkey.obj");
        m.enlarge(0.3f);
        m.rotate(0, 2.3f, 0);
        m.translate(0.1f, -0.1f, 1.6f);
        create_mesh(m, Material::create_standard(Texture::create_const_colour(Vec3(1, 1, 1)), 0));
        create_sphere(Vec3(-0.25f, -0.25f, 1.95f), 0.25f, Material::create_standard(Texture::create_const_colour(Vec3(0.8f, 0.8f, 0.8f)), 1));
    }
    /* texture_test_scene src/main.cu:189-204 */
    void texture_test_scene(const std::string &parsed_texture_filename = "textures/parsed_textures.txt")
    {
        create_cornell_box(Vec3(-0.5f, 0.5f, 1.2f), 1, 1, 1, 0.5f);
        ImageTexture earth("earth.png", parsed_texture_filename);
        create_sphere(Vec3(0, 0, 1.7f), 0.25f, Material::create_standard(earth.get_device_texture(), 0));
        Material tri_mat = Material::create_standard(Texture::create_checkerboard(Vec3(1, 1, 1), Vec3(0, 0, 0), 4), 0);
        create_triangle(Vertex{Vec3(0.1f, 0, 1.7f), Vec2(0, 0)}, Vertex{Vec3(0.6f, 0.5f, 1.9f), Vec2(0, 1)}, Vertex{Vec3(0.8f, 0.4f, 2), Vec2(1, 1)}, tri_mat);
    }
    void refract_test_scene()
    {   /* src/main.cu:206-213 */
        create_cornell_box(Vec3(-0.5f, 0.5f, 1.2f), 1, 1, 1, 0.5f);
        create_sphere(Vec3(0, -0.1f, 1.7f), 0.3f, Material::create_refractive(Texture::create_const_colour(Vec3(1, 1, 1)), 1.5f));
    }
    void reflection_test_scene()
    {   /* src/main.cu:172-187 */
        create_cornell_box(Vec3(-0.5f, 0.5f, 1.2f), 1, 1, 1, 0.5f);
        Texture t = Texture::create_const_colour(Vec3(1, 1, 1));
        create_sphere(Vec3(-0.2f, 0.2f, 1.7f), 0.15f, Material::create_standard(t, 0));
        create_sphere(Vec3(0.2f, 0.2f, 1.7f), 0.15f, Material::create_standard(t, 0.33f));
        create_sphere(Vec3(-0.2f, -0.2f, 1.7f), 0.15f, Material::create_standard(t, 0.66f));
        create_sphere(Vec3(0.2f, -0.2f, 1.7f), 0.15f, Material::create_standard(t, 1));
    }
};

/* src/camera.cu:32-108; assign_constant_mem() becomes the POD this object carries */
class Camera {
public:
    rt_camera c{};
    Camera(int width, int height) { rt_camera_default(width, height, &c); }                       /* pose constants of :34-41 */
    Camera(int width, int height, Vec3 pos, float fov, float focal_len, float x_rot, float y_rot, float z_rot)
    {
        rt_camera_make(width, height, pos.data(), fov, focal_len, x_rot, y_rot, z_rot, &c);
    }
    /* one thin-lens sample of this pinhole camera (rt_camera_lens): the image plane at focus_dist, the eye moved by (u, v) on the lens;
     * focal_len is what the camera was made with (0.1 for the default) */
    Camera lens(float focal_len, float focus_dist, float u, float v) const
    {
        Camera out(*this);
        if (rt_camera_lens(&c, focal_len, focus_dist, u, v, &out.c) != RT_OK) throw std::invalid_argument("bad lens parameters");
        return out;
    }
};

/* n lens samples of `cam` on a disc of radius `aperture`, by the golden-angle spiral r = aperture * sqrt((i + 0.5) / n),
 * theta = i * 2.39996323: rendered with Renderer::render_views(..., accumulate = true) they give one depth-of-field frame */
inline std::vector<Camera> lens_cameras(const Camera &cam, float focal_len, float focus_dist, float aperture, int n)
{
    std::vector<Camera> out;
    for (int i = 0; i < n; i++) {
        const double r = (double)aperture * std::sqrt(((double)i + 0.5) / (double)n), theta = (double)i * 2.39996323;
        out.push_back(cam.lens(focal_len, focus_dist, (float)(r * std::cos(theta)), (float)(r * std::sin(theta))));
    }
    return out;
}

/* src/raytracer.cu:4-12 with the defaults of RenderSettings src/main.cu:318-330 */
struct RenderData {
    rt_render_settings c{};
    RenderData(int rays_per_pixel = 100, int reflection_limit = 5, bool antialias = true, Vec3 sky_colour = Vec3(0, 0, 0))
    {
        c.rays_per_pixel = rays_per_pixel;
        c.reflection_limit = reflection_limit;
        c.antialias = antialias ? 1 : 0;
        c.sky_colour[0] = sky_colour.x; c.sky_colour[1] = sky_colour.y; c.sky_colour[2] = sky_colour.z;
    }
};

/* src/dispatch.cu:111-115 */
struct VariableRenderData {
    int frame_num;
    std::vector<float> previous_render;
};

/* A cube-map sky on a renderer's GPU (rt_sky_create; Renderer::create_sky makes one, Renderer::render_sky renders under it).  It must go
 * before the renderer it came from. */
class Sky {
public:
    Sky(Sky &&o) noexcept : h_(o.h_), face_size_(o.face_size_) { o.h_ = nullptr; }
    Sky(const Sky &) = delete;
    Sky &operator=(const Sky &) = delete;
    ~Sky() { rt_sky_destroy(h_); }
    const rt_sky *handle() const { return h_; }
    int face_size() const { return face_size_; }
    /* the direction through the centre of texel (face, row, col) of an n-face map (rt_sky_texel_direction): fill a map with any function of it */
    static Vec3 texel_direction(int face_size, int face, int row, int col)
    {
        float d[3];
        if (rt_sky_texel_direction(face_size, face, row, col, d) != RT_OK) throw std::invalid_argument("no such texel");
        return Vec3(d[0], d[1], d[2]);
    }

private:
    friend class Renderer;
    Sky(rt_sky *h, int face_size) : h_(h), face_size_(face_size) {}
    rt_sky *h_ = nullptr;
    int face_size_ = 0;
};

/* One GPU: owns the HIP context and the uploaded scene (replaces the __constant__ symbols and
 * allocate_constant_mem, src/dispatch.cu:104-108). */
class Renderer {
public:
    explicit Renderer(int device = 0)
    {
        rt_status st = rt_ctx_create(device, &ctx_);
        if (st == RT_ERR_NO_DEVICE) throw std::runtime_error("Error from HIP (creating context): no usable GPU; there is no CPU fallback");
        if (st != RT_OK) throw std::runtime_error("Error from HIP (creating context): status " + std::to_string(st));
    }
    ~Renderer()
    {
        rt_scene_destroy(scene_);
        rt_ctx_destroy(ctx_);
    }
    Renderer(const Renderer &) = delete;
    Renderer &operator=(const Renderer &) = delete;

    void set_scene(const SceneObjects &objs)
    {
        rt_scene_destroy(scene_);
        scene_ = nullptr;
        check(rt_scene_commit(ctx_, objs.handle(), &scene_));
    }
    /* The next time step of the scene: the mesh at object_index (the index of its create_mesh call among the scene's objects) gets new vertices,
     * nine floats per triangle in the order the mesh was committed with, as many triangles as it has.  Its BVH is rebuilt on the GPU; every later
     * render sees what a scene committed with these triangles would show (rt_scene_update_mesh). */
    void update_mesh(int object_index, const std::vector<float> &triangles)
    {
        if (triangles.size() % 9) throw std::invalid_argument("nine floats per triangle");
        check(rt_scene_update_mesh(ctx_, scene_, object_index, triangles.data(), (int32_t)(triangles.size() / 9)));
    }
    /* render(VariableRenderData*, int) src/dispatch.cu:156-163 */
    void render(const Camera &cam, const RenderData &rd, VariableRenderData *data, int current_time_ms)
    {
        if (data->previous_render.size() != (size_t)cam.c.width * (size_t)cam.c.height * 3) throw std::invalid_argument("previous_render has the wrong size");
        int32_t fn = data->frame_num;
        check(rt_render(ctx_, scene_,&cam.c, &rd.c, current_time_ms, &fn, data->previous_render.data()));
        data->frame_num = fn;
    }
    /* several passes of the main loop body at once (src/main.cu:421-424, one seed per frame): the same
     * image as that many render() calls, but the frames overlap on the GPU (rt_render_frames) */
    void render_frames(const Camera &cam, const RenderData &rd, VariableRenderData *data, const std::vector<int> &times_ms)
    {
        if (data->previous_render.size() != (size_t)cam.c.width * (size_t)cam.c.height * 3) throw std::invalid_argument("previous_render has the wrong size");
        if (times_ms.empty()) return;
        std::vector<int32_t> t(times_ms.begin(), times_ms.end());
        int32_t fn = data->frame_num;
        check(rt_render_frames(ctx_, scene_, &cam.c, &rd.c, t.data(), (int32_t)t.size(), &fn, data->previous_render.data()));
        data->frame_num = fn;
    }
    /* Many views of the scene in launches of up to RT_VIEWS_MAX (rt_render_views): view i has the camera cams[i] and the seed times_ms[i].
     * accumulate false: returns cams.size() frames back to back, each what render() gives for its camera from frame 0.  accumulate true:
     * `data` must be given; view i is folded into it as progressive frame data->frame_num + i, and the frame is returned as well. */
    std::vector<float> render_views(const std::vector<Camera> &cams, const RenderData &rd, const std::vector<int> &times_ms, bool accumulate = false,
                                    VariableRenderData *data = nullptr)
    {
        if (cams.empty() || cams.size() != times_ms.size()) throw std::invalid_argument("one time per camera, at least one camera");
        if (accumulate && !data) throw std::invalid_argument("an accumulated sequence needs the frame it goes into");
        const size_t frame = (size_t)cams[0].c.width * (size_t)cams[0].c.height * 3;
        if (accumulate && data->previous_render.size() != frame) throw std::invalid_argument("previous_render has the wrong size");
        std::vector<rt_camera> c;
        for (const Camera &cam : cams) c.push_back(cam.c);
        std::vector<int32_t> t(times_ms.begin(), times_ms.end());
        if (accumulate) {
            int32_t fn = data->frame_num;
            check(rt_render_views(ctx_, scene_, c.data(), t.data(), (int32_t)c.size(), &rd.c, 1, &fn, data->previous_render.data()));
            data->frame_num = fn;
            return data->previous_render;
        }
        std::vector<float> frames(frame * cams.size());
        int32_t fn = 0;
        check(rt_render_views(ctx_, scene_, c.data(), t.data(), (int32_t)c.size(), &rd.c, 0, &fn, frames.data()));
        return frames;
    }
    /* A sky from faces[6][n][n][3] (faces +X, -X, +Y, -Y, +Z, -Z; rows; columns), copied to the GPU */
    Sky create_sky(int face_size, const std::vector<float> &faces_rgb)
    {
        if (face_size < 1 || faces_rgb.size() != (size_t)6 * (size_t)face_size * (size_t)face_size * 3) throw std::invalid_argument("faces must hold 6 * n * n * 3 floats");
        rt_sky *h = nullptr;
        check(rt_sky_create(ctx_, face_size, faces_rgb.data(), &h));
        return Sky(h, face_size);
    }
    /* render_views under a sky (rt_render_sky): a ray that leaves the scene takes its light from the map, tinted by rd's sky colour */
    std::vector<float> render_sky(const Sky &sky, const std::vector<Camera> &cams, const RenderData &rd, const std::vector<int> &times_ms, bool accumulate = false,
                                  VariableRenderData *data = nullptr)
    {
        if (cams.empty() || cams.size() != times_ms.size()) throw std::invalid_argument("one time per camera, at least one camera");
        if (accumulate && !data) throw std::invalid_argument("an accumulated sequence needs the frame it goes into");
        const size_t frame = (size_t)cams[0].c.width * (size_t)cams[0].c.height * 3;
        if (accumulate && data->previous_render.size() != frame) throw std::invalid_argument("previous_render has the wrong size");
        std::vector<rt_camera> c;
        for (const Camera &cam : cams) c.push_back(cam.c);
        std::vector<int32_t> t(times_ms.begin(), times_ms.end());
        if (accumulate) {
            int32_t fn = data->frame_num;
            check(rt_render_sky(ctx_, scene_, sky.handle(), c.data(), t.data(), (int32_t)c.size(), &rd.c, 1, &fn, data->previous_render.data()));
            data->frame_num = fn;
            return data->previous_render;
        }
        std::vector<float> frames(frame * cams.size());
        int32_t fn = 0;
        check(rt_render_sky(ctx_, scene_, sky.handle(), c.data(), t.data(), (int32_t)c.size(), &rd.c, 0, &fn, frames.data()));
        return frames;
    }
    float last_kernel_ms()
    {
        float ms = 0;
        check(rt_last_kernel_ms(ctx_, &ms));
        return ms;
    }
    /* The closest hit of every ray (rt_trace_rays; get_ray_collision src/raytracer.cu:24-46 with the hit written out): origins and
     * directions hold n x 3 floats, the direction is taken as it is (not normalised).  A miss has object -1 and t RT_HIT_MISS_T. */
    std::vector<rt_hit> trace_rays(const std::vector<float> &origins, const std::vector<float> &directions)
    {
        if (origins.size() != directions.size() || origins.size() % 3 != 0) throw std::invalid_argument("origins and directions must hold n x 3 floats each");
        std::vector<rt_hit> hits(origins.size() / 3);
        check(rt_trace_rays(ctx_, scene_, origins.data(), directions.data(), (int64_t)hits.size(), hits.data()));
        return hits;
    }
    rt_hit trace_ray(Vec3 origin, Vec3 direction)
    {
        rt_hit h;
        check(rt_trace_rays(ctx_, scene_, origin.data(), direction.data(), 1, &h));
        return h;
    }
    /* The closest surface point of the scene for every point (rt_nearest_points): points holds n x 3 floats; max_dist n limits, or none
     * (unbounded).  The distance is unsigned.  A miss - nothing within the limit - has object -1 and distance RT_HIT_MISS_T. */
    std::vector<rt_nearest> nearest_points(const std::vector<float> &points, const std::vector<float> &max_dist = {})
    {
        if (points.size() % 3 != 0) throw std::invalid_argument("points must hold n x 3 floats");
        std::vector<rt_nearest> out(points.size() / 3);
        if (!max_dist.empty() && max_dist.size() != out.size()) throw std::invalid_argument("max_dist must hold n floats, or none");
        check(rt_nearest_points(ctx_, scene_, points.data(), max_dist.empty() ? nullptr : max_dist.data(), (int64_t)out.size(), out.data()));
        return out;
    }
    rt_nearest nearest_point(Vec3 point, float max_dist = INFINITY)
    {
        rt_nearest r;
        check(rt_nearest_points(ctx_, scene_, point.data(), &max_dist, 1, &r));
        return r;
    }
    /* Where a ball first touches the scene (rt_sweep_spheres): origins and directions hold n x 3 floats (a direction is taken as given: t is
     * in units of its length), radius n floats, tmax n limits on t, or none.  A miss - nothing within the limit, or an input that is not
     * valid - has object -1 and t RT_HIT_MISS_T; a ball that touches the scene at the start has overlap 1 and t 0. */
    std::vector<rt_sweep> sweep_spheres(const std::vector<float> &origins, const std::vector<float> &directions, const std::vector<float> &radius,
                                        const std::vector<float> &tmax = {})
    {
        if (origins.size() % 3 != 0 || directions.size() != origins.size()) throw std::invalid_argument("origins and directions must hold n x 3 floats each");
        std::vector<rt_sweep> out(origins.size() / 3);
        if (radius.size() != out.size()) throw std::invalid_argument("radius must hold n floats");
        if (!tmax.empty() && tmax.size() != out.size()) throw std::invalid_argument("tmax must hold n floats, or none");
        check(rt_sweep_spheres(ctx_, scene_, origins.data(), directions.data(), radius.data(), tmax.empty() ? nullptr : tmax.data(), (int64_t)out.size(), out.data()));
        return out;
    }
    rt_sweep sweep_sphere(Vec3 origin, Vec3 direction, float radius, float tmax = INFINITY)
    {
        rt_sweep r;
        check(rt_sweep_spheres(ctx_, scene_, origin.data(), direction.data(), &radius, &tmax, 1, &r));
        return r;
    }
    /* The generalized winding number of every point (rt_winding_numbers): points holds n x 3 floats; object an index of the scene's object
     * list, or RT_WINDING_SOLIDS for the sum over its spheres, cuboids and meshes.  1 (or -1) inside a closed surface, 0 outside. */
    std::vector<float> winding_numbers(const std::vector<float> &points, int32_t object = RT_WINDING_SOLIDS)
    {
        if (points.size() % 3 != 0) throw std::invalid_argument("points must hold n x 3 floats");
        std::vector<float> w(points.size() / 3);
        check(rt_winding_numbers(ctx_, scene_, points.data(), (int64_t)w.size(), object, w.data(), nullptr));
        return w;
    }
    /* Which points lie inside: 1 where |winding number| >= 0.5 */
    std::vector<uint8_t> contains(const std::vector<float> &points, int32_t object = RT_WINDING_SOLIDS)
    {
        if (points.size() % 3 != 0) throw std::invalid_argument("points must hold n x 3 floats");
        std::vector<uint8_t> in(points.size() / 3);
        check(rt_winding_numbers(ctx_, scene_, points.data(), (int64_t)in.size(), object, nullptr, in.data()));
        return in;
    }
    /* The signed distance of every point (rt_signed_distance): negative inside the scene's solids; max_dist n limits, or none.  `records`,
     * if given, receives the nearest-surface records the magnitudes come from. */
    std::vector<float> signed_distance(const std::vector<float> &points, const std::vector<float> &max_dist = {}, std::vector<rt_nearest> *records = nullptr)
    {
        if (points.size() % 3 != 0) throw std::invalid_argument("points must hold n x 3 floats");
        std::vector<float> sdf(points.size() / 3);
        if (!max_dist.empty() && max_dist.size() != sdf.size()) throw std::invalid_argument("max_dist must hold n floats, or none");
        if (records) records->resize(sdf.size());
        check(rt_signed_distance(ctx_, scene_, points.data(), max_dist.empty() ? nullptr : max_dist.data(), (int64_t)sdf.size(), records ? records->data() : nullptr,
                                 sdf.data()));
        return sdf;
    }
    /* winding_numbers through the meshes' dipole cluster trees (rt_winding_numbers_fast): far clusters of triangles answer with their dipole.
     * beta > 0 (infinity allowed): the larger, the closer to the exact answer and the slower.  Pays on meshes of thousands of triangles. */
    std::vector<float> winding_numbers_fast(const std::vector<float> &points, int32_t object = RT_WINDING_SOLIDS, float beta = RT_WINDING_BETA_DEFAULT)
    {
        if (points.size() % 3 != 0) throw std::invalid_argument("points must hold n x 3 floats");
        std::vector<float> w(points.size() / 3);
        check(rt_winding_numbers_fast(ctx_, scene_, points.data(), (int64_t)w.size(), object, beta, w.data(), nullptr));
        return w;
    }
    /* signed_distance with the sign from the fast winding numbers (rt_signed_distance_fast) */
    std::vector<float> signed_distance_fast(const std::vector<float> &points, float beta = RT_WINDING_BETA_DEFAULT, const std::vector<float> &max_dist = {},
                                            std::vector<rt_nearest> *records = nullptr)
    {
        if (points.size() % 3 != 0) throw std::invalid_argument("points must hold n x 3 floats");
        std::vector<float> sdf(points.size() / 3);
        if (!max_dist.empty() && max_dist.size() != sdf.size()) throw std::invalid_argument("max_dist must hold n floats, or none");
        if (records) records->resize(sdf.size());
        check(rt_signed_distance_fast(ctx_, scene_, points.data(), max_dist.empty() ? nullptr : max_dist.data(), (int64_t)sdf.size(), beta,
                                      records ? records->data() : nullptr, sdf.data()));
        return sdf;
    }
    /* The first k hits of every ray in order along it (rt_trace_rays_multi): origins, directions hold n x 3 floats, tmax n limits or none;
     * k from 1 to RT_MULTIHIT_MAX.  hits holds n * k records, [ray][rank], the ones behind a ray's last hit being misses; counts the records
     * each ray has. */
    struct MultiHits {
        std::vector<rt_hit> hits;
        std::vector<int32_t> counts;
    };
    MultiHits trace_rays_multi(const std::vector<float> &origins, const std::vector<float> &directions, int k, const std::vector<float> &tmax = {})
    {
        if (origins.size() != directions.size() || origins.size() % 3 != 0) throw std::invalid_argument("origins and directions must hold n x 3 floats each");
        if (k < 1 || k > RT_MULTIHIT_MAX) throw std::invalid_argument("k must be 1 .. RT_MULTIHIT_MAX (count_hits counts without records)");
        const size_t n = origins.size() / 3;
        if (!tmax.empty() && tmax.size() != n) throw std::invalid_argument("tmax must hold n floats, or none");
        MultiHits out;
        out.hits.resize(n * (size_t)k);
        out.counts.resize(n);
        check(rt_trace_rays_multi(ctx_, scene_, origins.data(), directions.data(), tmax.empty() ? nullptr : tmax.data(), (int64_t)n, k, out.hits.data(), out.counts.data()));
        return out;
    }
    /* How many surfaces every ray meets within its limit (rt_trace_rays_multi in count-only mode; a sphere counts once) */
    std::vector<int32_t> count_hits(const std::vector<float> &origins, const std::vector<float> &directions, const std::vector<float> &tmax = {})
    {
        if (origins.size() != directions.size() || origins.size() % 3 != 0) throw std::invalid_argument("origins and directions must hold n x 3 floats each");
        std::vector<int32_t> counts(origins.size() / 3);
        if (!tmax.empty() && tmax.size() != counts.size()) throw std::invalid_argument("tmax must hold n floats, or none");
        check(rt_trace_rays_multi(ctx_, scene_, origins.data(), directions.data(), tmax.empty() ? nullptr : tmax.data(), (int64_t)counts.size(), 0, nullptr, counts.data()));
        return counts;
    }
    /* Which surfaces touch every axis-aligned, closed box (rt_overlap_boxes): lo, hi hold n x 3 floats; k from 0 to RT_OVERLAP_MAX.  counts
     * holds, per box, the number of ALL surfaces - spheres and triangle records - that overlap it; ids n * k records, [box][rank], the k of
     * them lowest in (object, triangle) order, {-1, -1} behind a box's last.  A box that is not finite or has lo > hi overlaps nothing;
     * a sphere is a surface: a box wholly inside it does not touch it. */
    struct Overlaps {
        std::vector<int32_t> counts;
        std::vector<rt_overlap_id> ids;
    };
    Overlaps overlap_boxes(const std::vector<float> &lo, const std::vector<float> &hi, int k = 0)
    {
        if (lo.size() != hi.size() || lo.size() % 3 != 0) throw std::invalid_argument("lo and hi must hold n x 3 floats each");
        if (k < 0 || k > RT_OVERLAP_MAX) throw std::invalid_argument("k must be 0 .. RT_OVERLAP_MAX");
        const size_t n = lo.size() / 3;
        Overlaps out;
        out.counts.resize(n);
        out.ids.resize(n * (size_t)k);
        check(rt_overlap_boxes(ctx_, scene_, lo.data(), hi.data(), (int64_t)n, k, k > 0 ? out.ids.data() : nullptr, out.counts.data(), nullptr));
        return out;
    }
    /* Whether any surface touches every box (rt_overlap_boxes in any-only mode: a box stops at its first overlapping surface): 1 or 0 */
    std::vector<uint8_t> touches(const std::vector<float> &lo, const std::vector<float> &hi)
    {
        if (lo.size() != hi.size() || lo.size() % 3 != 0) throw std::invalid_argument("lo and hi must hold n x 3 floats each");
        std::vector<uint8_t> any(lo.size() / 3);
        check(rt_overlap_boxes(ctx_, scene_, lo.data(), hi.data(), (int64_t)any.size(), 0, nullptr, nullptr, any.data()));
        return any;
    }
    /* Which surfaces every query triangle cuts (rt_overlap_triangles): triangles holds n x 9 floats, the vertices a0, a1, a2; k from 0 to
     * RT_OVERLAP_MAX.  counts and ids as in overlap_boxes; with `segments` (needs k > 0) segments holds n * k records beside the ids: kind 1
     * a segment from p to q that the pair shares, kind 2 a sphere or a coplanar pair (no segment), kind 0 an empty slot.  A triangle that
     * is not finite overlaps nothing. */
    struct TriangleOverlaps {
        std::vector<int32_t> counts;
        std::vector<rt_overlap_id> ids;
        std::vector<rt_tri_segment> segments;
    };
    TriangleOverlaps overlap_triangles(const std::vector<float> &triangles, int k = 0, bool segments = false)
    {
        if (triangles.size() % 9 != 0) throw std::invalid_argument("triangles must hold n x 9 floats");
        if (k < 0 || k > RT_OVERLAP_MAX) throw std::invalid_argument("k must be 0 .. RT_OVERLAP_MAX");
        if (segments && k == 0) throw std::invalid_argument("segments need k > 0");
        const size_t n = triangles.size() / 9;
        TriangleOverlaps out;
        out.counts.resize(n);
        out.ids.resize(n * (size_t)k);
        if (segments) out.segments.resize(n * (size_t)k);
        check(rt_overlap_triangles(ctx_, scene_, triangles.data(), (int64_t)n, k, k > 0 ? out.ids.data() : nullptr, out.counts.data(), nullptr,
                                   segments ? out.segments.data() : nullptr));
        return out;
    }
    /* Whether the triangle (a0, a1, a2) cuts any surface (rt_overlap_triangles in any-only mode) */
    bool touches(Vec3 a0, Vec3 a1, Vec3 a2)
    {
        const float t[9] = {a0.x, a0.y, a0.z, a1.x, a1.y, a1.z, a2.x, a2.y, a2.z};
        uint8_t any = 0;
        check(rt_overlap_triangles(ctx_, scene_, t, 1, 0, nullptr, nullptr, &any, nullptr));
        return any != 0;
    }
    /* The first-hit planes of a view (rt_render_aov), all five of them: depth W*H, normal / albedo / ray W*H*3, object W*H */
    struct Aov {
        std::vector<float> depth, normal, albedo, ray;
        std::vector<int32_t> object;
    };
    Aov render_aov(const Camera &cam, Vec3 sky_colour = Vec3(0, 0, 0))
    {
        const size_t px = (size_t)cam.c.width * (size_t)cam.c.height;
        Aov a;
        a.depth.resize(px); a.normal.resize(px * 3); a.albedo.resize(px * 3); a.ray.resize(px * 3); a.object.resize(px);
        check(rt_render_aov(ctx_, scene_, &cam.c, sky_colour.data(), a.depth.data(), a.normal.data(), a.albedo.data(), a.object.data(), a.ray.data()));
        return a;
    }
    /* Is anything in the way (rt_occluded_rays)?  One byte per ray: 1 where the closest hit exists and lies at t <= tmax (in units of the
     * direction's length), else 0.  An empty tmax means "any hit at all". */
    std::vector<uint8_t> occluded_rays(const std::vector<float> &origins, const std::vector<float> &directions, const std::vector<float> &tmax = {})
    {
        if (origins.size() != directions.size() || origins.size() % 3 != 0) throw std::invalid_argument("origins and directions must hold n x 3 floats each");
        std::vector<uint8_t> out(origins.size() / 3);
        if (!tmax.empty() && tmax.size() != out.size()) throw std::invalid_argument("tmax must hold n floats, or none");
        check(rt_occluded_rays(ctx_, scene_, origins.data(), directions.data(), tmax.empty() ? nullptr : tmax.data(), (int64_t)out.size(), out.data()));
        return out;
    }
    bool occluded(Vec3 origin, Vec3 direction, float tmax = RT_HIT_MISS_T)
    {
        uint8_t b = 0;
        check(rt_occluded_rays(ctx_, scene_, origin.data(), direction.data(), &tmax, 1, &b));
        return b != 0;
    }
    /* The light-visibility plane of a view (rt_render_visibility): W*H bytes of RT_VIS_BLOCKED / RT_VIS_LIT / RT_VIS_NO_SURFACE */
    std::vector<uint8_t> render_visibility(const Camera &cam, Vec3 light_pos, float bias = 1e-3f)
    {
        std::vector<uint8_t> out((size_t)cam.c.width * (size_t)cam.c.height);
        check(rt_render_visibility(ctx_, scene_, &cam.c, light_pos.data(), bias, out.data()));
        return out;
    }
    /* The ambient-occlusion plane of a view (rt_render_ao): per pixel `samples` cosine-weighted directions from the first hit, each free
     * if nothing lies within `radius`; ao W*H floats (free / samples, 1 where there is no surface), count W*H (RT_AO_NO_SURFACE there) */
    struct Ao {
        std::vector<float> ao;
        std::vector<uint16_t> count;
    };
    Ao render_ao(const Camera &cam, int32_t samples = 16, float radius = RT_HIT_MISS_T, float bias = 1e-3f, int32_t time_ms = 0)
    {
        const size_t px = (size_t)cam.c.width * (size_t)cam.c.height;
        Ao a;
        a.ao.resize(px); a.count.resize(px);
        check(rt_render_ao(ctx_, scene_, &cam.c, samples, radius, bias, time_ms, a.count.data(), a.ao.data()));
        return a;
    }
    /* The edge-avoiding a-trous filter (rt_denoise) on a frame and the view's first-hit planes: colour W*H*3 floats (e.g.
     * previous_render), the planes as render_aov gives them.  The colour is divided by the albedo before the filter and multiplied
     * after (use_albedo), taps across an object edge are skipped (use_object).  Returns the filtered W*H*3 floats. */
    static rt_denoise_params denoise_defaults()
    {
        rt_denoise_params p;
        rt_denoise_params_default(&p);
        return p;
    }
    std::vector<float> denoise(const Camera &cam, const std::vector<float> &colour, const Aov &aov, const rt_denoise_params &params = denoise_defaults(),
                               bool use_object = true, bool use_albedo = true)
    {
        const size_t px = (size_t)cam.c.width * (size_t)cam.c.height;
        if (colour.size() != px * 3 || aov.normal.size() != px * 3 || aov.depth.size() != px || aov.object.size() != px || aov.albedo.size() != px * 3)
            throw std::invalid_argument("the frame and the planes must be of the camera's size");
        std::vector<float> out(px * 3);
        check(rt_denoise(ctx_, cam.c.width, cam.c.height, colour.data(), aov.normal.data(), aov.depth.data(), use_object ? aov.object.data() : nullptr,
                         use_albedo ? aov.albedo.data() : nullptr, &params, out.data()));
        return out;
    }
    /* Per-pixel sample budgets (rt_render_budget): pixel i takes budget[i] samples (0: it is left alone) and their mean is folded into
     * acc->frame by sample counts, acc->count growing by the budget; an accumulation starts as Accumulation(cam).  tile_list: only these
     * 8x8 tiles, in this order.  rd.c.rays_per_pixel is not read. */
    struct Accumulation {
        std::vector<float> frame;        /* W*H*3 */
        std::vector<uint32_t> count;     /* W*H: the samples each pixel's value holds */
        Accumulation() = default;
        explicit Accumulation(const Camera &cam) : frame((size_t)cam.c.width * (size_t)cam.c.height * 3, 0.0f), count((size_t)cam.c.width * (size_t)cam.c.height, 0u) {}
    };
    void render_budget(const Camera &cam, const RenderData &rd, const std::vector<uint16_t> &budget, Accumulation *acc, int time_ms, const std::vector<uint32_t> *tile_list = nullptr)
    {
        const size_t px = (size_t)cam.c.width * (size_t)cam.c.height;
        if (budget.size() != px || acc->frame.size() != px * 3 || acc->count.size() != px) throw std::invalid_argument("the budget and the accumulation must be of the camera's size");
        rt_tile_spec ts{};
        const uint32_t none = 0;
        if (tile_list) {
            ts.band_rows = 8; ts.band_stride = 1;
            ts.tile_list = tile_list->empty() ? &none : tile_list->data();
            ts.num_tiles = (int32_t)tile_list->size();
        }
        check(rt_render_budget(ctx_, scene_, &cam.c, &rd.c, time_ms, tile_list ? &ts : nullptr, budget.data(), acc->count.data(), acc->frame.data()));
    }
    /* The adaptive loop (rt_render_adaptive_host): a pilot, then passes that sample only where two half buffers of the view still disagree.
     * Returns the frame, the samples every pixel got and what the loop did. */
    static rt_adaptive_params adaptive_defaults()
    {
        rt_adaptive_params p;
        rt_adaptive_params_default(&p);
        return p;
    }
    struct Adaptive {
        std::vector<float> frame;
        std::vector<uint32_t> count;
        rt_adaptive_stats stats;
    };
    Adaptive render_adaptive(const Camera &cam, const RenderData &rd, int time_ms, const rt_adaptive_params &params = adaptive_defaults())
    {
        const size_t px = (size_t)cam.c.width * (size_t)cam.c.height;
        Adaptive a;
        a.frame.resize(px * 3); a.count.resize(px);
        std::memset(&a.stats, 0, sizeof a.stats);
        check(rt_render_adaptive_host(ctx_, scene_, &cam.c, &rd.c, time_ms, &params, a.frame.data(), a.count.data(), &a.stats));
        return a;
    }
    /* The main loop (src/main.cu:415-431) with frames in flight: submit_frame(get_time()) queues a frame and returns at once,
     * collect_frame() waits for the OLDEST submitted frame and blends it into data like render() would have.  With `depth`
     * frames submitted ahead the GPU stays full although every frame is seeded when it is submitted (rt_frame_submit):
     *     r.set_frames_in_flight(4);
     *     for (;;) { while (r.frames_in_flight() < 4) r.submit_frame(cam, rd, get_time()); r.collect_frame(&data); draw(data); }
     * The image after n collected frames is the image of n render() calls with the same seeds. */
    void set_frames_in_flight(int depth) { check(rt_frame_depth(ctx_, depth)); }
    int frames_in_flight() const { return rt_frames_pending(ctx_); }
    void submit_frame(const Camera &cam, const RenderData &rd, int current_time_ms) { check(rt_frame_submit(ctx_, scene_, &cam.c, &rd.c, current_time_ms, nullptr)); }
    void collect_frame(VariableRenderData *data)
    {
        int32_t fn = data->frame_num;
        check(rt_frame_collect_host(ctx_, &fn, data->previous_render.data()));
        data->frame_num = fn;
    }
    /* the camera moved (src/main.cu:392-407 restarts at frame 0): drop what is in flight */
    void discard_frames()
    {
        int32_t fn = 0;
        while (rt_frames_pending(ctx_) > 0) check(rt_frame_collect_host(ctx_, &fn, nullptr));
    }

private:
    rt_ctx *ctx_ = nullptr;
    rt_scene *scene_ = nullptr;
    void check(rt_status st)
    {
        if (st == RT_OK) return;
        std::string msg = rt_last_error(ctx_);
        if (st == RT_ERR_UNSUPPORTED) throw std::logic_error(msg);
        if (st == RT_ERR_INVALID) throw std::invalid_argument(msg);
        throw std::runtime_error(msg);                                  /* check_cuda_error src/utils.cu:5-10 */
    }
};

/* Several GPUs of one node behind the same render() (rt_render_multi): every device of `devices` renders the 8x8
 * tiles it owns - dealt out interleaved on the first call for a view, which measures them, and by measured cost
 * from the second on - and the tiles meet on devices[0].  The image is the single-GPU image bit for
 * bit (a pixel depends only on its coordinates, its seed and its previous value, src/raytracer.cu:118-131).
 * The reference is single-GPU; this is what its main loop calls when the node has more than one. */
class MultiRenderer {
public:
    explicit MultiRenderer(const std::vector<int> &devices)
    {
        if (devices.empty()) throw std::invalid_argument("no devices");
        for (int d : devices) {
            rt_ctx *c = nullptr;
            rt_status st = rt_ctx_create(d, &c);
            if (st != RT_OK) {
                release();
                if (st == RT_ERR_NO_DEVICE) throw std::runtime_error("Error from HIP (creating context): no usable GPU; there is no CPU fallback");
                throw std::runtime_error("Error from HIP (creating context): status " + std::to_string(st));
            }
            ranks_.push_back(rt_rank{c, nullptr});
        }
    }
    ~MultiRenderer() { release(); }
    MultiRenderer(const MultiRenderer &) = delete;
    MultiRenderer &operator=(const MultiRenderer &) = delete;

    int num_gpus() const { return (int)ranks_.size(); }
    /* every GPU holds the whole scene (it is tens of KB) */
    void set_scene(const SceneObjects &objs)
    {
        for (rt_rank &r : ranks_) {
            rt_scene_destroy(const_cast<rt_scene *>(r.scene));
            r.scene = nullptr;
            rt_scene *s = nullptr;
            check(r.ctx, rt_scene_commit(r.ctx, objs.handle(), &s));
            r.scene = s;
        }
    }
    /* render(VariableRenderData*, int) src/dispatch.cu:156-163 */
    void render(const Camera &cam, const RenderData &rd, VariableRenderData *data, int current_time_ms)
    {
        render_frames(cam, rd, data, std::vector<int>{current_time_ms});
    }
    void render_frames(const Camera &cam, const RenderData &rd, VariableRenderData *data, const std::vector<int> &times_ms)
    {
        if (data->previous_render.size() != (size_t)cam.c.width * (size_t)cam.c.height * 3) throw std::invalid_argument("previous_render has the wrong size");
        if (times_ms.empty()) return;
        std::vector<int32_t> t(times_ms.begin(), times_ms.end());
        int32_t fn = data->frame_num;
        check(ranks_[0].ctx, rt_render_multi(ranks_.data(), (int32_t)ranks_.size(), &cam.c, &rd.c, t.data(), (int32_t)t.size(), &fn, data->previous_render.data()));
        data->frame_num = fn;
    }
    /* does GPU i exchange its tiles with the first GPU directly (xGMI peer access), or staged by the runtime? */
    bool direct_peer_copies(int i) { return rt_peer_access(ranks_.at(0).ctx, ranks_.at((size_t)i).ctx) == 1; }
    /* the slowest rank's kernel time of the last call */
    float last_kernel_ms()
    {
        float worst = 0;
        for (rt_rank &r : ranks_) {
            float ms = 0;
            if (rt_last_kernel_ms(r.ctx, &ms) == RT_OK && ms > worst) worst = ms;
        }
        return worst;
    }

private:
    std::vector<rt_rank> ranks_;
    void release()
    {
        for (rt_rank &r : ranks_) {
            rt_scene_destroy(const_cast<rt_scene *>(r.scene));
            rt_ctx_destroy(r.ctx);
        }
        ranks_.clear();
    }
    static void check(rt_ctx *ctx, rt_status st)
    {
        if (st == RT_OK) return;
        std::string msg = rt_last_error(ctx);
        if (st == RT_ERR_UNSUPPORTED) throw std::logic_error(msg);
        if (st == RT_ERR_INVALID) throw std::invalid_argument(msg);
        throw std::runtime_error(msg);
    }
};

/* parse_pixel_colours src/main.cu:343-371: int(px*255), clamp, alpha 255 */
inline std::vector<uint8_t> parse_pixel_colours(const std::vector<float> &pixel_colours, int width, int height)
{
    std::vector<uint8_t> out((size_t)width * (size_t)height * 4);
    for (size_t i = 0; i < (size_t)width * (size_t)height; i++) {
        for (int k = 0; k < 3; k++) {
            /* a defined conversion (NaN -> 0, saturating), the same as rt_to_rgba8_device: a plain cast of a NaN or an
             * infinite value is undefined in C++ */
            const float scaled = pixel_colours[3 * i + k] * 255;
            int colour = scaled != scaled ? 0 : (scaled >= 2147483648.0f ? 2147483647 : (scaled <= -2147483648.0f ? -2147483647 - 1 : (int)scaled));
            if (colour > 255) colour = 255; else if (colour < 0) colour = 0;
            out[4 * i + k] = (uint8_t)colour;
        }
        out[4 * i + 3] = 255;
    }
    return out;
}

/* What the reference shows in its SFML window (src/main.cu:374-386) written to a file instead:
 * an 8-bit RGB PNG (the format of the reference's images/ directory) without any library - zlib
 * "stored" blocks, so the file is W*H*3 bytes plus headers. */
inline void write_png(const std::string &path, const std::vector<uint8_t> &rgba, int width, int height)
{
    auto crc32 = [](const uint8_t *p, size_t n, uint32_t crc) {
        crc = ~crc;
        for (size_t i = 0; i < n; i++) {
            crc ^= p[i];
            for (int k = 0; k < 8; k++) crc = (crc >> 1) ^ (0xedb88320u & (0u - (crc & 1u)));
        }
        return ~crc;
    };
    auto be32 = [](std::vector<uint8_t> &v, uint32_t x) { for (int s = 24; s >= 0; s -= 8) v.push_back((uint8_t)(x >> s)); };
    /* raw scanlines: filter byte 0 + RGB */
    std::vector<uint8_t> raw;
    raw.reserve((size_t)height * ((size_t)width * 3 + 1));
    for (int y = 0; y < height; y++) {
        raw.push_back(0);
        for (int x = 0; x < width; x++) {
            const uint8_t *px = &rgba[4 * ((size_t)y * (size_t)width + (size_t)x)];
            raw.push_back(px[0]); raw.push_back(px[1]); raw.push_back(px[2]);
        }
    }
    /* zlib stream of stored deflate blocks (at most 65535 bytes each) + adler32 */
    std::vector<uint8_t> z = {0x78, 0x01};
    uint32_t a = 1, b = 0;
    for (size_t off = 0; off < raw.size() || off == 0; off += 65535) {
        const size_t n = raw.size() - off < 65535 ? raw.size() - off : 65535;
        z.push_back(off + n >= raw.size() ? 1 : 0);
        z.push_back((uint8_t)(n & 255)); z.push_back((uint8_t)(n >> 8));
        z.push_back((uint8_t)(~n & 255)); z.push_back((uint8_t)((~n >> 8) & 255));
        z.insert(z.end(), raw.begin() + (std::ptrdiff_t)off, raw.begin() + (std::ptrdiff_t)(off + n));
        for (size_t i = off; i < off + n; i++) { a = (a + raw[i]) % 65521u; b = (b + a) % 65521u; }
        if (n == 0) break;
    }
    be32(z, (b << 16) | a);
    std::vector<uint8_t> file = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    auto chunk = [&](const char *type, const std::vector<uint8_t> &data) {
        be32(file, (uint32_t)data.size());
        const size_t start = file.size();
        file.insert(file.end(), type, type + 4);
        file.insert(file.end(), data.begin(), data.end());
        be32(file, crc32(&file[start], file.size() - start, 0));
    };
    std::vector<uint8_t> ihdr;
    be32(ihdr, (uint32_t)width); be32(ihdr, (uint32_t)height);
    ihdr.push_back(8); ihdr.push_back(2); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);   /* 8-bit RGB */
    chunk("IHDR", ihdr);
    chunk("IDAT", z);
    chunk("IEND", {});
    FILE *fp = std::fopen(path.c_str(), "wb");
    if (!fp) throw std::runtime_error("cannot open output file");
    const bool ok = std::fwrite(file.data(), 1, file.size(), fp) == file.size();
    std::fclose(fp);
    if (!ok) throw std::runtime_error("cannot write output file");
}

}  // namespace rtamd

#endif
