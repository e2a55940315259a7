/*
 * driver.cpp — runs the reference renderer's own sources on the CPU and dumps what they compute
 * (TEST INFRASTRUCTURE; built by oracle/ref_build.py into oracle/_ref/, one program per image size).
 *
 * The reference's translation unit is included below, from the build-time copy, with its `main`
 * renamed.  Everything this file calls is the reference's public interface: SceneObjects(0..3),
 * Texture::create_*, Material::create_*, Object::create_*, ObjFileMesh, Camera::assign_constant_mem,
 * allocate_constant_mem, render, get_ray_collision, parse_pixel_colours.  `private` is opened for that
 * one include so that the scene list, the transformed triangles and the BVH arrays can be written out;
 * no member is modified.
 *
 * usage: refdrv JOBFILE   — a job is a whitespace-separated command list:
 *   threads N
 *   builtin N                                   the reference's own SceneObjects(N), N in 0..3
 *   mat standard r g b s | mat gradient s | mat checkerboard lr lg lb dr dg db n s | mat image NAME s
 *     | mat emissive r g b strength | mat refractive r g b n        sets the material of the objects that follow
 *   sphere cx cy cz r | triangle 9f | triangle_uv 9f 6f | quad 12f | one_way_quad 12f invert
 *     | cuboid x y z w h d | mesh FILE n | obj FILE k {enlarge s | rotate x y z | translate x y z}*k
 *   commit                                      upload the scene built from the object commands
 *   settings spp limit antialias                RenderData (a builtin scene keeps its own sky colour)
 *   sky r g b
 *   reset                                       frame_num = 0, previous render = zeros
 *   render time_ms OUT                          one render() call (frame_num and the previous render carry over)
 *   camera OUT | rgba8 OUT | tris OBJECT OUT | bvh OBJECT OUTPREFIX | rays FILE n OUT | pixels FILE n OUT
 * Outputs are raw little-endian arrays; oracle/ref_driver.py wraps them.
 */
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <random>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "cuda_standin.h"

thread_local uint3 threadIdx, blockIdx;
thread_local dim3 blockDim, gridDim;

static int g_threads = 1;

/* what a <<<grid, block>>> launch does, on at most 16 host threads: every thread of every block runs the
 * kernel once with its indices set.  Blocks are handed out dynamically; pixels are independent. */
template <typename K, typename... A>
static void cpu_launch(K kernel, dim3 grid, dim3 block, A... args)
{
    const unsigned int nblocks = grid.x * grid.y * grid.z;
    std::atomic<unsigned int> next(0);
    auto work = [&]() {
        gridDim = grid;
        blockDim = block;
        for (unsigned int b = next++; b < nblocks; b = next++) {
            blockIdx.x = b % grid.x; blockIdx.y = (b / grid.x) % grid.y; blockIdx.z = b / (grid.x * grid.y);
            for (unsigned int z = 0; z < block.z; z++)
                for (unsigned int y = 0; y < block.y; y++)
                    for (unsigned int x = 0; x < block.x; x++) {
                        threadIdx.x = x; threadIdx.y = y; threadIdx.z = z;
                        kernel(args...);
                    }
        }
    };
    int n = g_threads < 1 ? 1 : (g_threads > 16 ? 16 : g_threads);
    std::vector<std::thread> pool;
    for (int i = 1; i < n; i++) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
}

/* `private` and `protected` are opened for the include below.  Every standard header the reference includes
 * (<cmath>, <vector>, <chrono>, <random>, <stdexcept>, <fstream>, and <string> through them) is included ABOVE, with
 * the keywords intact, so that inside the include their guards make them empty.  If the reference ever includes
 * another standard header, add it to the list above first: a library header parsed with the keywords redefined
 * can fail in obscure ways. */
#define main reference_main
#define private public
#define protected public
#include "src/main.cu"
#undef protected
#undef private
#undef main

struct Job {
    std::vector<std::string> tok;
    size_t pos = 0;
    bool more() const { return pos < tok.size(); }
    std::string word() { if (!more()) throw std::runtime_error("job file ends inside a command"); return tok[pos++]; }
    float f() { std::string w = word(); char *e; float v = strtof(w.c_str(), &e); if (*e) throw std::runtime_error("not a number: " + w); return v; }
    int i() { std::string w = word(); char *e; long v = strtol(w.c_str(), &e, 10); if (*e) throw std::runtime_error("not an integer: " + w); return (int)v; }
    Vec3 v3() { float x = f(), y = f(), z = f(); return Vec3(x, y, z); }
    Vec2 v2() { float x = f(), y = f(); return Vec2(x, y); }
};

static void dump(const std::string &path, const void *p, size_t n)
{
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp || (n && fwrite(p, 1, n, fp) != n)) throw std::runtime_error("cannot write " + path);
    fclose(fp);
}

static std::vector<float> slurp(const std::string &path, size_t nfloats)
{
    std::vector<float> v(nfloats);
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp || fread(v.data(), sizeof(float), nfloats, fp) != nfloats) throw std::runtime_error("cannot read " + path);
    fclose(fp);
    return v;
}

/* two materials as far as the reference's factories set them (every other field is zero under
 * -ftrivial-auto-var-init=zero): used only to tell which of several objects a RayCollision's material came from */
static bool same3(Vec3 a, Vec3 b) { return memcmp(&a, &b, sizeof a) == 0; }
static bool same_fields(Material &a, Material &b)
{
    return a.type == b.type && a.texture.type == b.texture.type && same3(a.texture.colour, b.texture.colour)
        && same3(a.texture.light, b.texture.light) && same3(a.texture.dark, b.texture.dark) && a.texture.num_squares == b.texture.num_squares
        && a.texture.img_rgb == b.texture.img_rgb && memcmp(&a.smoothness, &b.smoothness, 4) == 0 && a.need_uv == b.need_uv
        && same3(a.emitted_light, b.emitted_light) && memcmp(&a.refractive_index, &b.refractive_index, 4) == 0;
}

static void push3(std::vector<float> &o, Vec3 v) { o.push_back(v.x); o.push_back(v.y); o.push_back(v.z); }

static int run(Job &job)
{
    Camera camera;
    camera.assign_constant_mem();

    std::vector<Object> *objects = nullptr;          /* the scene list the dumps read (never the uploaded copy) */
    std::vector<Object> own;
    SceneObjects *builtin = nullptr, *helper = nullptr;
    bool use_sky = true;
    Material mat = Material::create_standard(Texture::create_const_colour(Vec3(0, 0, 0)), 0);
    RenderData settings{1, 1, true, Vec3(0, 0, 0)};
    VariableRenderData data{0, std::vector<float>(PIXEL_ARRAY_LEN, 0)};
    bool uploaded = false;

    auto upload = [&](AllObjects all) { allocate_constant_mem(settings, all); uploaded = true; };
    auto need_scene = [&]() { if (!uploaded) throw std::runtime_error("no scene: `builtin N` or `commit` first"); };
    auto object_at = [&](int k) -> Object & {
        need_scene();
        if (k < 0 || k >= (int)objects->size()) throw std::runtime_error("object index out of range");
        return (*objects)[k];
    };

    while (job.more()) {
        std::string c = job.word();
        if (c == "threads") g_threads = job.i();
        else if (c == "builtin") {
            builtin = new SceneObjects(job.i());
            objects = &builtin->objects;
            use_sky = builtin->use_sky;
            settings.sky_colour = use_sky ? SKY_COLOUR : Vec3(0, 0, 0);
            upload(builtin->gpu_struct);
        } else if (c == "mat") {
            std::string k = job.word();
            if (k == "standard") { Vec3 col = job.v3(); mat = Material::create_standard(Texture::create_const_colour(col), job.f()); }
            else if (k == "gradient") mat = Material::create_standard(Texture::create_gradient(), job.f());
            else if (k == "checkerboard") { Vec3 l = job.v3(), d = job.v3(); int n = job.i(); mat = Material::create_standard(Texture::create_checkerboard(l, d, n), job.f()); }
            else if (k == "image") { ImageTexture img(job.word()); mat = Material::create_standard(img.get_device_texture(), job.f()); }
            else if (k == "emissive") { Vec3 col = job.v3(); mat = Material::create_emissive(col, job.f()); }
            else if (k == "refractive") { Vec3 col = job.v3(); mat = Material::create_refractive(Texture::create_const_colour(col), job.f()); }
            else throw std::runtime_error("unknown material " + k);
        } else if (c == "sphere") { Vec3 p = job.v3(); own.push_back(Object::create_sphere(p, job.f(), mat)); }
        else if (c == "triangle") { Vec3 a = job.v3(), b = job.v3(), d = job.v3(); own.push_back(Object::create_triangle(a, b, d, mat)); }
        else if (c == "triangle_uv") {
            Vec3 a = job.v3(), b = job.v3(), d = job.v3();
            Vec2 ua = job.v2(), ub = job.v2(), ud = job.v2();
            own.push_back(Object::create_triangle(Vertex{a, ua}, Vertex{b, ub}, Vertex{d, ud}, mat));
        } else if (c == "quad") { Vec3 a = job.v3(), b = job.v3(), d = job.v3(), e = job.v3(); own.push_back(Object::create_quad(a, b, d, e, mat)); }
        else if (c == "one_way_quad") { Vec3 a = job.v3(), b = job.v3(), d = job.v3(), e = job.v3(); own.push_back(Object::create_one_way_quad(a, b, d, e, job.i() != 0, mat)); }
        else if (c == "cuboid") { Vec3 p = job.v3(); float w = job.f(), h = job.f(), d = job.f(); own.push_back(Object::create_cuboid(p, w, h, d, mat)); }
        else if (c == "mesh") {
            std::string path = job.word();
            int n = job.i();
            std::vector<float> v = slurp(path, (size_t)n * 9);
            std::vector<Triangle> tris;
            for (int t = 0; t < n; t++) {
                const float *p = &v[(size_t)t * 9];
                /* a named local, as in the reference's own create_mesh: -ftrivial-auto-var-init=zero then makes the
                 * texture points this constructor leaves unset the zeros the project defines */
                Triangle tri(Vec3(p[0], p[1], p[2]), Vec3(p[3], p[4], p[5]), Vec3(p[6], p[7], p[8]), mat);
                tris.push_back(tri);
            }
            ReadOnlyDeviceArray<Triangle> device_array(tris);
            own.push_back(Object::create_mesh(tris, device_array.device_pointer, mat));
        } else if (c == "obj") {
            ObjFileMesh m(job.word());
            for (int k = job.i(); k > 0; k--) {
                std::string t = job.word();
                if (t == "enlarge") m.enlarge(job.f());
                else if (t == "rotate") { float x = job.f(), y = job.f(), z = job.f(); m.rotate(x, y, z); }
                else if (t == "translate") { float x = job.f(), y = job.f(), z = job.f(); m.translate(x, y, z); }
                else throw std::runtime_error("unknown transform " + t);
            }
            if (!helper) helper = new SceneObjects(1);       /* only for its faces -> triangles -> mesh method */
            own.push_back(helper->create_mesh(m, mat));
        } else if (c == "commit") {
            objects = &own;
            ReadOnlyDeviceArray<Object> array(own);
            upload(AllObjects{array.device_pointer, (int)own.size()});
        } else if (c == "settings") {
            settings.rays_per_pixel = job.i();
            settings.reflection_limit = job.i();
            settings.antialias = job.i() != 0;
            cudaMemcpyToSymbol(const_render_data, &settings, sizeof(settings));
        } else if (c == "sky") {
            settings.sky_colour = job.v3();
            cudaMemcpyToSymbol(const_render_data, &settings, sizeof(settings));
        } else if (c == "reset") {
            data.frame_num = 0;
            data.previous_render.assign(PIXEL_ARRAY_LEN, 0);
        } else if (c == "render") {
            need_scene();
            int time_ms = job.i();
            render(&data, time_ms);
            dump(job.word(), data.previous_render.data(), sizeof(float) * data.previous_render.size());
        } else if (c == "camera") {
            dump(job.word(), &const_cam_data, sizeof(const_cam_data));
        } else if (c == "rgba8") {
            std::vector<sf::Uint8> px = parse_pixel_colours(data.previous_render);
            dump(job.word(), px.data(), px.size());
        } else if (c == "tris") {
            Object &o = object_at(job.i());
            std::vector<float> out;
            for (Triangle &t : o.mesh.host_triangles) for (int k = 0; k < 3; k++) push3(out, t.points[k]);
            dump(job.word(), out.data(), sizeof(float) * out.size());
        } else if (c == "bvh") {
            Object &o = object_at(job.i());
            std::string prefix = job.word();
            BVH &b = o.mesh.bvh;
            std::vector<float> boxes;
            std::vector<int> links, list;
            for (size_t k = 0; k < b.data_array.size(); k++) {
                push3(boxes, b.data_array[k].box.bl_near);
                push3(boxes, b.data_array[k].box.tr_far);
                links.push_back(b.left_pointer[k]);
                links.push_back(b.right_pointer[k]);
                links.push_back(b.data_array[k].num_tris);
                for (int t = 0; t < b.data_array[k].num_tris; t++) list.push_back(b.data_array[k].device_tri_inxs[t]);
            }
            links.push_back(b.root_node_inx);
            dump(prefix + ".boxes", boxes.data(), sizeof(float) * boxes.size());
            dump(prefix + ".links", links.data(), sizeof(int) * links.size());
            dump(prefix + ".list", list.data(), sizeof(int) * list.size());
        } else if (c == "rays" || c == "pixels") {
            /* rays: FILE holds n x (origin, direction) floats.  pixels: FILE holds n x (x, y) ints and each ray is the
             * reference's own primary ray of that pixel (antialias off).  Per ray 17 words: origin, direction, then
             * hit flag (int), object (int), distance, hit point, normal, texture uv.  The reference's record names
             * no object but carries the winner's MATERIAL (RayCollision::hit_mesh_material): the object written is
             * the one whose own hit() returns the winning distance and whose material is the returned one.  Where
             * that does not single one out (objects tied in distance with equal materials) it is the last of the
             * tied ones; OUT.info counts those rays, and the rays with a distance tie at all. */
            need_scene();
            std::string path = job.word();
            int n = job.i();
            bool pixels = c == "pixels";
            std::vector<float> in = slurp(path, (size_t)n * (pixels ? 2 : 6));
            std::vector<float> out((size_t)n * 17);
            int ties = 0, ambiguous = 0;
            for (int r = 0; r < n; r++) {
                uint state = 0;
                int px = 0, py = 0;
                if (pixels) { memcpy(&px, &in[(size_t)r * 2], 4); memcpy(&py, &in[(size_t)r * 2 + 1], 4); }
                Ray ray(px, py, &state, false);
                if (!pixels) {
                    const float *p = &in[(size_t)r * 6];
                    ray.origin = Vec3(p[0], p[1], p[2]);
                    ray.change_direction(Vec3(p[3], p[4], p[5]));
                }
                RayCollision col = get_ray_collision(&ray);
                int object = -1;
                if (col.hit_data.ray_hits) {
                    int tied = 0, same_material = 0, by_material = -1, last_tied = -1;
                    for (int k = 0; k < const_objects.num_meshes; k++) {
                        RayHitData h = const_objects.meshes[k].hit(&ray);
                        if (!h.ray_hits || h.ray_travelled_dist != col.hit_data.ray_travelled_dist) continue;
                        tied++;
                        last_tied = k;
                        if (same_fields(const_objects.meshes[k].material, col.hit_mesh_material)) { same_material++; by_material = k; }
                    }
                    object = same_material == 1 ? by_material : last_tied;
                    if (same_material != 1) ambiguous++;
                    if (tied > 1) ties++;
                }
                float *o = &out[(size_t)r * 17];
                o[0] = ray.origin.x; o[1] = ray.origin.y; o[2] = ray.origin.z;
                o[3] = ray.direction.x; o[4] = ray.direction.y; o[5] = ray.direction.z;
                o += 6;
                int flag = col.hit_data.ray_hits ? 1 : 0;
                memcpy(o, &flag, 4);
                memcpy(o + 1, &object, 4);
                o[2] = col.hit_data.ray_travelled_dist;
                o[3] = col.hit_data.hit_point.x; o[4] = col.hit_data.hit_point.y; o[5] = col.hit_data.hit_point.z;
                o[6] = col.hit_data.normal_vec.x; o[7] = col.hit_data.normal_vec.y; o[8] = col.hit_data.normal_vec.z;
                o[9] = col.hit_data.texture_uv.x; o[10] = col.hit_data.texture_uv.y;
            }
            std::string path_out = job.word();
            dump(path_out, out.data(), sizeof(float) * out.size());
            int counts[2] = {ties, ambiguous};
            dump(path_out + ".info", counts, sizeof(counts));
        } else throw std::runtime_error("unknown command " + c);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s JOBFILE  (image size %dx%d)\n", argv[0], SCREEN_WIDTH, SCREEN_HEIGHT); return 2; }
    try {
        Job job;
        std::ifstream in(argv[1]);
        if (!in) throw std::runtime_error(std::string("cannot open ") + argv[1]);
        for (std::string w; in >> w;) job.tok.push_back(w);
        return run(job);
    } catch (const std::exception &e) {
        fprintf(stderr, "refdrv: %s\n", e.what());
        return 1;
    }
}
