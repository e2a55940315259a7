// The sub-entry words (ray-tracer_amd/csrc/rt_entry.h, "The sub-entry words": rt_sub_cone_of, rt_sub_index, rt_entry_word on the sub-cone)
// against the traversal they speak for, on the CPU under AddressSanitizer + UndefinedBehaviorSanitizer (test infrastructure;
// tests/test_primary_subentry.py writes the scenes, compiles and runs it).  The scene files, the rays, the two walks and their comparison
// are entry_soundness.cpp's, taken from it as they are (its main is set aside); what is new here is which cone a word is computed for and
// which jitters it is held against.
//   subentry_soundness scene FILE [seed] [draws]   every jittered view of FILE: every pixel that wants a table (unflagged, own word 0), every
//                                                  sub-box with a non-zero word, at the 27 corners, edge midpoints, face centres and centre of
//                                                  the sub-box - its ends are the thresholds -J/2, 0, J/2 and +-J themselves, so a threshold is
//                                                  held against both neighbouring sub-boxes' words -, at -0.0f where the sub-box holds 0, and at
//                                                  `draws` random jitters; each also against the word rt_sub_index picks for it, which is what the
//                                                  kernel reads.  Prints the share of sub-boxes resolved, plain and weighted by the centre ray's
//                                                  gated node steps.
//   subentry_soundness adversarial [seed] [trees]  entry_soundness.cpp's one-node trees, the word computed for the sub-cone the extreme draw falls
//                                                  in.  Built with -DRT_ENTRY_E=0.0 this mode finds a counter-example; with the margins, none.
//   subentry_soundness index                       rt_sub_axis_index against a brute-force search of the closed sub-intervals for every float
//                                                  within 4096 ulp of each threshold and of +-J, and a coarse sweep of [-J, J]; monotone
//   subentry_soundness encoding                    no slot word reads as `triangle`, `nothing` or 0; the layout's regions do not overlap
//   subentry_soundness complete FILE               with cap forced to 0 and to 1 a pixel without a slot keeps 0: the kernel's two-step write
//                                                  (compaction, then refinement) replayed on an array of rt_sub_alloc_words words
//   subentry_soundness plan [seed]                 rt_cull_host::Plan with the larger allocation: same view, changed view, scene revision, growth,
//                                                  a refused allocation, and the threshold policy
#define main entry_soundness_main
#include "entry_soundness.cpp"
#undef main

static uint32_t sub_word_of(const Scene &s, const float P[3], const float cam[12], uint32_t idx) { return word_of(s, rt_sub_cone_of(P, cam, idx)); }

static bool valid_word(const Scene &s, uint32_t w) { return w == 0u || w == RT_ENTRY_NOTHING || ((w & RT_ENTRY_TAG) && (w >> 1) < (uint32_t)s.num_tris); }

static bool read_scene(FILE *f, Scene &s, int32_t head[7])
{
    bool ok = std::fread(head, 4, 7, f) == 7 && head[0] > 0 && head[0] < (1 << 24);
    if (!ok) return false;
    s.blob.resize((size_t)head[0] * 4);
    s.off_nodes = head[1]; s.num_nodes = head[2]; s.off_meshes = head[3]; s.off_tris = head[4]; s.num_tris = head[5];
    ok = std::fread(s.blob.data(), 4, s.blob.size(), f) == s.blob.size();
    return ok && s.off_nodes >= 0 && s.num_nodes >= 0 && s.off_nodes + 4 * s.num_nodes <= head[0] && s.off_meshes >= 0 && s.off_meshes + 2 <= head[0] && s.off_tris >= 0 &&
           s.num_tris >= 0 && s.off_tris + 3 * s.num_tris <= head[0];
}

// entry_soundness.cpp's same() for the sub-box's own word and the word the index picks, the walk from the root done once
static bool same_both(const Scene &s, const Ray &r, uint32_t own, uint32_t picked, const float P[3], long long it)
{
    const Outcome plain = walk_root(s, r);
    uint32_t bp;
    std::memcpy(&bp, &plain.best, 4);
    for (int k = 0; k < 2; k++) {
        const uint32_t word = k == 0 ? own : picked;
        if (word == 0u || (k == 1 && picked == own)) continue;
        const Outcome entry = walk_entry(s, r, word);
        uint32_t be;
        std::memcpy(&be, &entry.best, 4);
        if (plain.steps >= 0 && bp == be && plain.prim == entry.prim && (word != RT_ENTRY_NOTHING || plain.prim == -1)) continue;
        return same(s, r, word, P, it);         // (reports it)
    }
    return true;
}

// does the closed sub-box idx hold the jitter?
static bool in_sub_box(uint32_t idx, const float off[3])
{
    for (int k = 0; k < 3; k++) {
        const int j = (int)((idx >> (2 * k)) & 3u);
        if (!(off[k] >= rt_sub_tau(j) && off[k] <= rt_sub_tau(j + 1))) return false;
    }
    return true;
}

static int run_sub_scene(const char *path, uint64_t seed, int random_draws)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    int32_t head[7];
    Scene s;
    bool ok = read_scene(f, s, head);
    long long rays = 0, tables = 0, n_tri = 0, n_nothing = 0, n_zero = 0, steps_resolved = 0, steps_all = 0;
    for (int view = 0; ok && view < head[6]; view++) {
        float cam[12];
        int32_t size[2];
        ok = std::fread(cam, 4, 12, f) == 12 && std::fread(size, 4, 2, f) == 2 && size[0] > 0 && size[1] > 0 && size[0] * size[1] <= (1 << 20);
        if (!ok) break;
        g_rng.seed(seed * 1000 + (uint64_t)view);
        long long view_tables = 0;
        for (int py = 0; py < size[1]; py++)
            for (int px = 0; px < size[0]; px++) {
                float P[3];
                rt_cull_primary(cam, px, py, P);
                const rt_cull_cone cone = rt_cull_cone_of(P, cam, 1);
                const bool flagged = rt_cull_no_leaf(cone, s.blob.data(), s.off_nodes, s.num_nodes, s.off_meshes, 1, rt_cull_local_stack());
                const uint32_t own = word_of(s, cone);
                if (!rt_sub_wants_table(flagged, own)) {
                    if (!flagged && own == 0u) { std::fprintf(stderr, "pixel (%d, %d): unflagged with the word 0, and no table\n", px, py); std::fclose(f); return 1; }
                    continue;
                }
                if (flagged || own != 0u) { std::fprintf(stderr, "pixel (%d, %d): a table for a flagged pixel or one with the word %08x\n", px, py, own); std::fclose(f); return 1; }
                // (a pixel that finds the image's tables full keeps 0 and has no sub-words: the first rt_sub_cap in pixel order stand for those the device picks)
                if ((size_t)view_tables >= rt_sub_cap(rt_cull_words(size[0], size[1]))) continue;
                view_tables++;
                tables++;
                uint32_t table[RT_SUB_WORDS];
                for (uint32_t idx = 0; idx < RT_SUB_WORDS; idx++) {
                    table[idx] = sub_word_of(s, P, cam, idx);
                    if (!valid_word(s, table[idx])) {
                        std::fprintf(stderr, "pixel (%d, %d) sub-box %u: the word %08x is neither 0 nor `nothing` nor a tagged triangle of the mesh\n", px, py, idx, table[idx]);
                        std::fclose(f);
                        return 1;
                    }
                }
                const uint32_t gates = rt_cull_gate_word(cone, s.blob.data(), s.off_nodes, s.num_nodes, s.off_meshes, 0, rt_cull_local_stack());
                const float inv[3] = {1.0f / P[0], 1.0f / P[1], 1.0f / P[2]};
                long long centre = rt_cull_walk_steps(s.blob.data(), s.off_nodes, s.num_nodes, s.off_meshes, 0, cam, P, inv, gates);
                if (centre < 0) centre = 0;
                for (uint32_t idx = 0; idx < RT_SUB_WORDS; idx++) {
                    steps_all += centre;
                    if (table[idx] == 0u) { n_zero++; continue; }
                    steps_resolved += centre;
                    (table[idx] == RT_ENTRY_NOTHING ? n_nothing : n_tri)++;
                    float lo[3], hi[3];
                    bool zero[3];
                    for (int k = 0; k < 3; k++) {
                        const int j = (int)((idx >> (2 * k)) & 3u);
                        lo[k] = rt_sub_tau(j); hi[k] = rt_sub_tau(j + 1);
                        zero[k] = lo[k] <= 0.0f && hi[k] >= 0.0f;
                    }
                    // 27 points of the sub-box, 7 with a -0.0f in them where the sub-box holds 0, then random draws
                    const int draws = 27 + 7 + random_draws;
                    for (int k = 0; k < draws; k++) {
                        float off[3];
                        for (int a = 0; a < 3; a++) {
                            const int which = k < 27 ? (a == 0 ? k % 3 : a == 1 ? (k / 3) % 3 : k / 9) : 3;
                            off[a] = which == 0 ? lo[a] : which == 2 ? hi[a] : which == 1 ? 0.5f * (lo[a] + hi[a]) : (float)urand(lo[a], hi[a]);
                            if (off[a] < lo[a]) off[a] = lo[a];
                            if (off[a] > hi[a]) off[a] = hi[a];
                            if (k >= 27 && k < 34 && (((k - 26) >> a) & 1) && zero[a]) off[a] = -0.0f;
                        }
                        if (!in_sub_box(idx, off)) { std::fprintf(stderr, "a draw left its sub-box\n"); std::fclose(f); return 1; }
                        const Ray r = ray_of(P, cam, off, true);
                        rays++;
                        // the sub-box's own word, and the word the kernel would read for this jitter (another one only on a threshold)
                        const uint32_t picked = table[rt_sub_index(off[0], off[1], off[2])];
                        if (!in_sub_box(rt_sub_index(off[0], off[1], off[2]), off)) { std::fprintf(stderr, "rt_sub_index picks a sub-box that does not hold the jitter\n"); std::fclose(f); return 1; }
                        if (!same_both(s, r, table[idx], picked, P, rays)) {
                            std::fprintf(stderr, "  view %d pixel (%d, %d) sub-box %u jitter %a %a %a\n", view, px, py, idx, off[0], off[1], off[2]);
                            std::fclose(f);
                            return 1;
                        }
                    }
                }
            }
    }
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "%s is not a scene file\n", path); return 2; }
    std::printf("subentry soundness: %lld rays over %d views, %lld tables, sub-words: %lld triangle, %lld nothing, %lld not known; resolved share %.4f, step-weighted %.4f; "
                "no counter-example, sanitizers silent\n", rays, head[6], tables, n_tri, n_nothing, n_zero,
                tables ? (double)(n_tri + n_nothing) / (double)(tables * RT_SUB_WORDS) : 0.0, steps_all ? (double)steps_resolved / (double)steps_all : 0.0);
    return 0;
}

// entry_soundness.cpp's one-node trees (its run_adversarial, restated: that one computes the word of the whole cone), the word computed for
// the sub-cone of the extreme draw
static int run_sub_adversarial(uint64_t seed, long long trees)
{
    g_rng.seed(seed);
    Scene s;
    s.off_meshes = 0; s.off_nodes = 2; s.num_nodes = 1; s.off_tris = 6; s.num_tris = 2;
    s.blob.assign(4 * (6 + 6), 0.0f);
    long long n_tri = 0, n_nothing = 0, n_zero = 0;
    for (long long it = 0; it < trees; it++) {
        float cam[12], P[3];
        const float scale = (float)std::pow(10.0, urand(-1, 1));
        for (int k = 0; k < 3; k++) cam[k] = (float)urand(-3, 3) * scale;
        const int W = irand(8, 2000), H = irand(8, 1200);
        double fw[3] = {urand(-1, 1), urand(-1, 1), urand(-1, 1)}, up[3] = {urand(-1, 1), urand(-1, 1), urand(-1, 1)};
        double rr[3] = {fw[1] * up[2] - fw[2] * up[1], fw[2] * up[0] - fw[0] * up[2], fw[0] * up[1] - fw[1] * up[0]};
        double u2[3] = {rr[1] * fw[2] - rr[2] * fw[1], rr[2] * fw[0] - rr[0] * fw[2], rr[0] * fw[1] - rr[1] * fw[0]};
        const double nf = std::sqrt(fw[0] * fw[0] + fw[1] * fw[1] + fw[2] * fw[2]) + 1e-9, nr = std::sqrt(rr[0] * rr[0] + rr[1] * rr[1] + rr[2] * rr[2]) + 1e-9,
                     nu = std::sqrt(u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]) + 1e-9;
        const double focal = urand(0.05, 1.0), half = focal * std::tan(urand(0.2, 0.8)), step = 2 * half / W;
        for (int k = 0; k < 3; k++) {
            cam[6 + k] = (float)(rr[k] / nr * step);
            cam[9 + k] = (float)(-u2[k] / nu * step);
            cam[3 + k] = (float)(cam[k] + fw[k] / nf * focal - rr[k] / nr * half + u2[k] / nu * half * H / W);
        }
        rt_cull_primary(cam, irand(0, W - 1), irand(0, H - 1), P);
        // a corner of a sub-box: the ray is then a corner of the sub-cone, where the range of a linear form is attained
        const uint32_t idx = (uint32_t)irand(0, RT_SUB_WORDS - 1);
        float off[3];
        for (int k = 0; k < 3; k++) off[k] = rt_sub_tau((int)((idx >> (2 * k)) & 3u) + irand(0, 1));
        const Ray ray = ray_of(P, cam, off, true);
        if (ray.nan) continue;
        const float t = (float)std::pow(10.0, urand(-1, 1)) * scale;
        float X[3];
        for (int k = 0; k < 3; k++) X[k] = ray.o[k] + ray.d[k] * t;
        float *m = s.blob.data(), *n = s.blob.data() + 4 * 2, *tr = s.blob.data() + 4 * 6;
        const int mode = irand(0, 2);
        {
            float *q = tr;
            float e1[3], e2[3];
            for (int k = 0; k < 3; k++) { e1[k] = (float)urand(-0.3, 0.3) * t; e2[k] = (float)urand(-0.3, 0.3) * t; }
            const float a = (float)urand(0.2, 0.7), b = mode == 0 ? 0.0f : (float)urand(0.1, 0.25);
            for (int k = 0; k < 3; k++) {
                q[k] = X[k] - a * e2[k] - b * e1[k];
                if (mode == 0) q[k] = ulps(q[k], irand(-4, 4));
                q[3 + k] = e1[k]; q[6 + k] = e2[k];
            }
        }
        {
            float *q = tr + 12;
            const bool behind = irand(0, 2) != 0;
            float e1[3], e2[3];
            for (int k = 0; k < 3; k++) { e1[k] = (float)urand(-1, 1) * t; e2[k] = (float)urand(-1, 1) * t; }
            for (int k = 0; k < 3; k++) {
                const float Y = ray.o[k] + ray.d[k] * t * (behind ? 1.5f : 1.0f) + (behind ? 0.0f : (float)urand(2, 3) * t);
                q[k] = Y - 0.3f * e1[k] - 0.3f * e2[k];
                q[3 + k] = e1[k]; q[6 + k] = e2[k];
            }
        }
        float b0[2][3], b1[2][3];
        for (int c = 0; c < 2; c++) {
            const float *q = tr + 12 * c;
            for (int k = 0; k < 3; k++) {
                const float v0 = q[k], v1 = q[k] + q[3 + k], v2 = q[k] + q[6 + k];
                const float pad = (float)urand(0, 0.05) * t;
                b0[c][k] = fminf(v0, fminf(v1, v2)) - pad; b1[c][k] = fmaxf(v0, fmaxf(v1, v2)) + pad;
            }
        }
        if (mode == 1 && ray.d[0] != 0.0f && ray.d[1] != 0.0f && ray.d[2] != 0.0f) {
            const int j = irand(0, 2), i = (j + irand(1, 2)) % 3;
            const float far_plane = ray.d[j] > 0 ? b1[0][j] : b0[0][j];
            const float tj = (far_plane - ray.o[j]) * ray.inv[j];
            const float at = ulps(ray.o[i] + tj * ray.d[i], irand(-6, 6));
            if (ray.d[i] > 0) b0[0][i] = at; else b1[0][i] = at;
            if (b0[0][i] > b1[0][i]) { const float x = b0[0][i]; b0[0][i] = b1[0][i]; b1[0][i] = x; }
        }
        for (int k = 0; k < 3; k++) { m[k] = fminf(b0[0][k], b0[1][k]) - 0.01f * t; m[3 + k] = fmaxf(b1[0][k], b1[1][k]) + 0.01f * t; }
        const uint32_t root = 0u, lref = RT_REF_LEAF | (1u << RT_REF_COUNT_SHIFT) | 0u, rref = RT_REF_LEAF | (1u << RT_REF_COUNT_SHIFT) | 1u, lgate = 2u, rgate = 4u;
        std::memcpy(&m[6], &root, 4);
        for (int c = 0; c < 2; c++)
            for (int k = 0; k < 3; k++) { n[6 * c + k] = b0[c][k]; n[6 * c + 3 + k] = b1[c][k]; }
        std::memcpy(&n[12], &lref, 4); std::memcpy(&n[13], &rref, 4); std::memcpy(&n[14], &lgate, 4); std::memcpy(&n[15], &rgate, 4);
        const uint32_t word = sub_word_of(s, P, cam, idx);
        if (word == 0u) { n_zero++; continue; }
        (word == RT_ENTRY_NOTHING ? n_nothing : n_tri)++;
        if (!same(s, ray, word, P, it)) return 1;
    }
    std::printf("subentry soundness, adversarial: %lld one-node trees, sub-words: %lld triangle, %lld nothing, %lld not known; no counter-example, sanitizers silent\n", trees,
                n_tri, n_nothing, n_zero);
    return 0;
}

// the closed sub-intervals that hold x, as a bit set
static unsigned brute_intervals(float x)
{
    unsigned set = 0;
    for (int j = 0; j < RT_SUB_S; j++)
        if (x >= rt_sub_tau(j) && x <= rt_sub_tau(j + 1)) set |= 1u << j;
    return set;
}

static int run_index()
{
    auto fail = [](const char *what, float x) { std::fprintf(stderr, "index: %s at %a\n", what, x); return 1; };
    if (rt_sub_tau(0) != -RT_CULL_JITTER || rt_sub_tau(4) != RT_CULL_JITTER || rt_sub_tau(1) * 2.0f != -RT_CULL_JITTER || rt_sub_tau(3) * 2.0f != RT_CULL_JITTER || rt_sub_tau(2) != 0.0f)
        return fail("the thresholds are not -J, -J/2, 0, J/2, J", 0.0f);
    if (rt_jitter(0u) != -RT_CULL_JITTER || rt_jitter(0xffffffffu) != RT_CULL_JITTER) return fail("rt_jitter's range is not [-J, J]", 0.0f);
    long long checked = 0;
    for (int j = 0; j <= RT_SUB_S; j++) {
        // every float within 4096 ulp of the threshold, inside [-J, J]
        float x = ulps(rt_sub_tau(j), -4096);
        uint32_t last = 0;
        for (int k = 0; k <= 8192; k++, x = std::nextafterf(x, INFINITY)) {
            if (x < -RT_CULL_JITTER || x > RT_CULL_JITTER) continue;
            const uint32_t i = rt_sub_axis_index(x);
            if (i > 3u || !(brute_intervals(x) & (1u << i))) return fail("the index names a sub-interval that does not hold the jitter", x);
            if (i < last) return fail("the index is not monotone", x);
            last = i;
            checked++;
        }
    }
    if (rt_sub_axis_index(-0.0f) != rt_sub_axis_index(0.0f) || !(brute_intervals(-0.0f) & (1u << rt_sub_axis_index(-0.0f)))) return fail("-0.0f", -0.0f);
    uint32_t last = 0;
    for (int k = 0; k <= 2000000; k++) {
        const float x = rt_jitter((uint32_t)((uint64_t)k * 0xffffffffull / 2000000ull));
        const uint32_t i = rt_sub_axis_index(x);
        if (i > 3u || !(brute_intervals(x) & (1u << i))) return fail("the index names a sub-interval that does not hold the jitter", x);
        if (i < last) return fail("the index is not monotone over rt_jitter's range", x);
        last = i;
        checked++;
    }
    for (uint32_t idx = 0; idx < RT_SUB_WORDS; idx++) {
        const float c[3] = {0.5f * (rt_sub_tau((int)(idx & 3u)) + rt_sub_tau((int)(idx & 3u) + 1)), 0.5f * (rt_sub_tau((int)((idx >> 2) & 3u)) + rt_sub_tau((int)((idx >> 2) & 3u) + 1)),
                            0.5f * (rt_sub_tau((int)(idx >> 4)) + rt_sub_tau((int)(idx >> 4) + 1))};
        if (rt_sub_index(c[0], c[1], c[2]) != idx) return fail("the centre of a sub-box has another index: jx + 4 jy + 16 jz", c[0]);
    }
    std::printf("subentry index: %lld floats, every index names a closed sub-interval that holds its jitter, monotone; sanitizers silent\n", checked);
    return 0;
}

static int run_encoding()
{
    auto fail = [](const char *what) { std::fprintf(stderr, "encoding: %s\n", what); return 1; };
    const uint32_t slots[] = {0u, 1u, 2u, 3u, 62u, 63u, 64u, 259199u, (1u << 25) - 1u};
    for (uint32_t slot : slots) {
        const uint32_t w = rt_sub_slot_word(slot);
        if (w == 0u || w == RT_ENTRY_NOTHING || (w & RT_ENTRY_TAG)) return fail("a slot word reads as 0, `nothing` or `triangle`");
        if (rt_sub_slot_plus1(w) != slot + 1u) return fail("a slot does not come back out of its word");
    }
    if (rt_sub_slot_plus1(0u) || rt_sub_slot_plus1(RT_ENTRY_NOTHING)) return fail("0 or `nothing` carries a slot");
    for (uint32_t t = 0; t < 100000u; t += 7u)
        if (rt_sub_slot_plus1(rt_entry_triangle(t))) return fail("a `triangle` word carries a slot");
    if (!rt_sub_wants_table(false, 0u) || rt_sub_wants_table(true, 0u) || rt_sub_wants_table(false, RT_ENTRY_NOTHING) || rt_sub_wants_table(false, rt_entry_triangle(5u)))
        return fail("only an unflagged pixel whose word is 0 wants a table");
    // what a table stores: the sub-word comes back out, a stored gate word is no `triangle` and no `nothing`, and every bit of it but bit 0 survives
    const uint32_t gate_words[] = {0u, 2u, 0xfffffffeu, 0x80000000u, 0x12345678u};
    for (uint32_t g : gate_words) {
        if (rt_sub_word_of(rt_sub_stored(0u, g)) != 0u || rt_sub_stored(0u, g) != g) return fail("a sub-box that is not known does not store the pixel's gate word");
        if (rt_sub_word_of(rt_sub_stored(RT_ENTRY_NOTHING, g)) != RT_ENTRY_NOTHING || rt_sub_stored(RT_ENTRY_NOTHING, g) == g) return fail("`nothing` does not survive its storage");
        for (uint32_t t = 0; t <= RT_REF_START_MASK; t += 4099u)
            if (rt_sub_stored(rt_entry_triangle(t), g) != rt_entry_triangle(t) || rt_sub_word_of(rt_entry_triangle(t)) != rt_entry_triangle(t) || rt_entry_triangle(t) == RT_SUB_NOTHING)
                return fail("a `triangle` word does not survive its storage");
    }
    for (size_t words : {(size_t)2, (size_t)194, (size_t)64800}) {
        if (rt_sub_header_base(words) != rt_cull_alloc_words_entry(words) || rt_sub_pixels_base(words) != rt_sub_header_base(words) + RT_SUB_HEADER ||
            rt_sub_tables_base(words) != rt_sub_pixels_base(words) + rt_sub_cap(words) || rt_sub_alloc_words(words) != rt_sub_tables_base(words) + rt_sub_cap(words) * RT_SUB_WORDS)
            return fail("the regions behind the entry words overlap or leave a gap");
        if (rt_sub_cap(words) * 8 != words * 32) return fail("cap is not an eighth of the pre-pass's threads");
    }
    std::printf("subentry encoding: slot words, the regions; sanitizers silent\n");
    return 0;
}

// the device's two steps restated on a host array: the compaction in pixel order with `cap` slots, then the refinement of the slots handed out.
// This shares rt_sub_wants_table, rt_sub_slot_word and the layout functions with rt_sub_compact_kernel, not the kernel's own branches: it holds the
// layout and the encoding to "a pixel without a slot keeps 0", and would not see a wrong full-table branch in the kernel.  That branch runs in
// tests/test_gpu_primary_subentry.py's narrow-field-of-view case, where more pixels want a table than the image holds: the tables in use are
// min(wanting, cap), each table pixel's own word reads 0 through rt_debug_primary_entry, and the frame is the oracle's.
static int run_complete(const char *path)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    int32_t head[7];
    Scene s;
    float cam[12];
    int32_t size[2];
    const bool ok = read_scene(f, s, head) && head[6] > 0 && std::fread(cam, 4, 12, f) == 12 && std::fread(size, 4, 2, f) == 2 && size[0] > 0 && size[1] > 0 && size[0] * size[1] <= (1 << 20);
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "%s is not a scene file\n", path); return 2; }
    const int W = size[0], H = size[1];
    const size_t words = rt_cull_words(W, H);
    long long wanting = 0;
    for (long long cap : {0ll, 1ll, (long long)rt_sub_cap(words)}) {
        std::vector<uint32_t> plane(rt_sub_alloc_words(words), 0xdeadbeefu);
        uint32_t &counter = plane[rt_sub_header_base(words)];
        counter = 0u;
        wanting = 0;
        for (int i = 0; i < W * H; i++) {
            float P[3];
            rt_cull_primary(cam, i % W, i / W, P);
            const rt_cull_cone cone = rt_cull_cone_of(P, cam, 1);
            const bool flagged = rt_cull_no_leaf(cone, s.blob.data(), s.off_nodes, s.num_nodes, s.off_meshes, 1, rt_cull_local_stack());
            uint32_t &entry = plane[rt_cull_entry_base(words) + (size_t)i];
            entry = flagged ? 0u : word_of(s, cone);
            if (!rt_sub_wants_table(flagged, entry)) continue;
            wanting++;
            const uint32_t slot = counter++;
            if ((long long)slot < cap) { plane[rt_sub_pixels_base(words) + slot] = (uint32_t)i; entry = rt_sub_slot_word(slot); }
            else entry = 0u;
        }
        const long long handed = (long long)counter < cap ? (long long)counter : cap;
        for (long long slot = 0; slot < handed; slot++) {
            const uint32_t i = plane[rt_sub_pixels_base(words) + (size_t)slot];
            float P[3];
            rt_cull_primary(cam, (int)i % W, (int)i / W, P);
            for (uint32_t idx = 0; idx < RT_SUB_WORDS; idx++) plane[rt_sub_tables_base(words) + (size_t)slot * RT_SUB_WORDS + idx] = sub_word_of(s, P, cam, idx);
        }
        long long with_slot = 0;
        for (int i = 0; i < W * H; i++) {
            const uint32_t entry = plane[rt_cull_entry_base(words) + (size_t)i], s1 = rt_sub_slot_plus1(entry);
            if (s1 == 0u) continue;
            with_slot++;
            if ((long long)s1 > handed || plane[rt_sub_pixels_base(words) + s1 - 1u] != (uint32_t)i) { std::fprintf(stderr, "complete: pixel %d carries a slot that is not its own\n", i); return 1; }
        }
        if (with_slot != handed || handed != (wanting < cap ? wanting : cap)) { std::fprintf(stderr, "complete: cap %lld: %lld pixels carry a slot, %lld handed out, %lld want one\n", cap, with_slot, handed, wanting); return 1; }
    }
    if (wanting < 2) { std::fprintf(stderr, "complete: the view has fewer than two pixels that want a table\n"); return 1; }
    std::printf("subentry complete: %lld pixels want a table; with cap 0 and 1 the others keep 0; sanitizers silent\n", wanting);
    return 0;
}

// rt_cull_host::Plan with the tables behind the plane
static int run_sub_plan(uint64_t seed)
{
    g_rng.seed(seed);
    using rt_cull_host::Step;
    rt_cull_host::Plan plan;
    std::vector<uint32_t> device;
    long long grows = 0, refinements = 0;
    size_t refuse_above = (size_t)-1;
    auto grow = [&](size_t words) {
        grows++;
        const size_t n = plan.tables ? rt_sub_alloc_words(words) : rt_cull_alloc_words_entry(words);
        if (n > refuse_above) { device.clear(); device.shrink_to_fit(); return false; }
        device.assign(n, 0xdeadbeefu);
        return true;
    };
    // what the pre-pass and the refinement write: the last word of each region
    auto pre_pass = [&](const rt_cull_host::Key &k) { device[rt_cull_alloc_words_entry(rt_cull_words(k.width, k.height)) - 1] = 0u; };
    auto refinement = [&](const rt_cull_host::Key &k) { refinements++; device[rt_sub_alloc_words(rt_cull_words(k.width, k.height)) - 1] = 0u; };
    auto fail = [](const char *what) { std::fprintf(stderr, "plan: %s\n", what); return 1; };
    // one launch of `samples` with the threshold 1000: returns whether it refined
    auto launch = [&](const rt_cull_host::Key &k, int64_t samples, Step want, bool &refined) {
        const Step st = plan.next(k, true, grow);
        if (st != want) return false;
        refined = plan.refine(st, k, samples, 1000);
        if (st == Step::run) { pre_pass(k); plan.ran(k, true); }
        if (refined) refinement(k);
        return true;
    };
    rt_cull_host::Key k;
    k.scene_uid = 7; k.width = 96; k.height = 64; k.antialias = 1;
    for (int i = 0; i < 12; i++) k.cam[i] = (float)i;
    bool r = false;
    // switched off: the old allocation, never a refinement
    plan.want_tables = false;
    if (!launch(k, 5000, Step::run, r) || r || plan.tables || device.size() != rt_cull_alloc_words_entry(rt_cull_words(96, 64))) return fail("switched off, a launch allocates or refines tables");
    if (!launch(k, 5000, Step::reuse, r) || r) return fail("switched off, a reuse refines");
    // switched on: the allocation grows to hold the tables although the image has not grown
    plan.want_tables = true;
    k.cam[3] += 1.0f;
    if (!launch(k, 999, Step::run, r) || r || !plan.tables || device.size() != rt_sub_alloc_words(rt_cull_words(96, 64)) || grows != 2) return fail("below the threshold: no refinement, but the larger allocation");
    if (!launch(k, 1, Step::reuse, r) || !r) return fail("the first reuse does not refine");
    if (!launch(k, 5000, Step::reuse, r) || r) return fail("the second reuse refines again");
    // a changed view at the threshold: at once, and not again
    k.cam[3] += 1.0f;
    if (!launch(k, 1000, Step::run, r) || !r) return fail("at the threshold the first launch does not refine");
    if (!launch(k, 1000, Step::reuse, r) || r) return fail("a view refined at once is refined again on reuse");
    // a scene revision: computed again, refined again
    k.scene_uid++;
    if (!launch(k, 10, Step::run, r) || r) return fail("a scene revision below the threshold refines at once");
    if (!launch(k, 10, Step::reuse, r) || !r) return fail("a scene revision is not refined on its first reuse");
    // a view without jitter: never
    k.antialias = 0;
    if (!launch(k, 5000, Step::run, r) || r) return fail("a view without jitter is refined");
    if (!launch(k, 5000, Step::reuse, r) || r) return fail("a view without jitter is refined on reuse");
    k.antialias = 1;
    // growth: a larger image, the tables with it; a smaller one: none
    k.width = 200; k.height = 131;
    const long long g0 = grows;
    if (!launch(k, 5000, Step::run, r) || !r || grows != g0 + 1 || device.size() != rt_sub_alloc_words(rt_cull_words(200, 131))) return fail("a larger image does not grow the tables");
    k.width = 37; k.height = 21;
    if (!launch(k, 5000, Step::run, r) || !r || grows != g0 + 1) return fail("a smaller image grows the allocation");
    for (int i = 0; i < 200; i++) {
        k.width = irand(1, 300); k.height = irand(1, 200); k.scene_uid += (uint32_t)irand(0, 1);
        const Step st = plan.next(k, true, grow);
        if (st == Step::none) return fail("a launch went without a plane");
        const bool ref = plan.refine(st, k, irand(0, 2000), 1000);
        if (st == Step::run) { pre_pass(k); plan.ran(k, true); }
        if (device.size() < rt_sub_alloc_words(rt_cull_words(k.width, k.height))) return fail("the allocation does not hold the view's tables");
        if (ref) refinement(k);
    }
    // the tables refused, the plane alone granted: the launch has its plane and nothing is refined, nor asked for again at this size
    k.width = 640; k.height = 480;
    refuse_above = rt_cull_alloc_words_entry(rt_cull_words(640, 480));
    const long long g1 = grows;
    if (!launch(k, 5000, Step::run, r) || r || plan.tables || grows != g1 + 2 || device.size() != rt_cull_alloc_words_entry(rt_cull_words(640, 480))) return fail("refused tables take the plane with them, or are refined");
    if (!launch(k, 5000, Step::reuse, r) || r) return fail("a plane without tables is refined on reuse");
    k.cam[3] += 1.0f;
    if (!launch(k, 5000, Step::run, r) || r || grows != g1 + 2) return fail("refused tables are asked for again at the same size");
    // everything refused: no plane; then granted again
    refuse_above = 0;
    k.width = 800; k.height = 600;
    if (plan.next(k, true, grow) != Step::none || plan.valid || plan.cap_words != 0 || plan.refine(Step::none, k, 5000, 1000)) return fail("a refused allocation leaves a plane behind");
    refuse_above = (size_t)-1;
    if (!launch(k, 5000, Step::run, r) || !r || !plan.tables) return fail("the launch after a refused allocation does not get its plane and tables");
    // a refinement that could not be queued: the view is computed again
    k.cam[3] += 1.0f;
    if (!launch(k, 10, Step::run, r) || r) return fail("setup");
    if (plan.next(k, true, grow) != Step::reuse || !plan.refine(Step::reuse, k, 10, 1000)) return fail("setup: the reuse does not refine");
    plan.refine_failed();
    if (!launch(k, 10, Step::run, r) || r) return fail("after a failed refinement the view is not computed again");
    std::printf("subentry plan: %lld allocations, %lld refinements; sanitizers silent\n", grows, refinements);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !std::strcmp(argv[1], "scene")) return run_sub_scene(argv[2], argc > 3 ? strtoull(argv[3], nullptr, 10) : 1, argc > 4 ? atoi(argv[4]) : 8);
    if (argc >= 2 && !std::strcmp(argv[1], "adversarial")) return run_sub_adversarial(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1, argc > 3 ? atoll(argv[3]) : 300000);
    if (argc >= 2 && !std::strcmp(argv[1], "index")) return run_index();
    if (argc >= 2 && !std::strcmp(argv[1], "encoding")) return run_encoding();
    if (argc >= 3 && !std::strcmp(argv[1], "complete")) return run_complete(argv[2]);
    if (argc >= 2 && !std::strcmp(argv[1], "plan")) return run_sub_plan(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
    std::fprintf(stderr, "usage: subentry_soundness scene FILE [seed] [draws] | adversarial [seed] [trees] | index | encoding | complete FILE | plan [seed]\n");
    (void)entry_soundness_main;
    return 2;
}
