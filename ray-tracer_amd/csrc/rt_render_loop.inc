/*
 * rt_render_loop.inc — the body of the render kernel: included by rt_render_kernel.h once per kernel that runs the wave loop, behind the
 * head of what runs it (template <int NT, bool HAS_MESH, int MODE> ... (ARGS a)), with RT_LOOP_BUDGET defined as false (rt_render_kernel,
 * rt_views_loop, rt_sky_loop) or true (rt_budget_loop), RT_LOOP_VIEWS as true (rt_views_loop, rt_sky_loop: a camera per frame of the launch) or
 * false, RT_LOOP_SKY as true (rt_sky_loop: a miss looks the sky up in a cube map) or false and RT_LOOP_TRAITS as the scene traits the kernel is
 * compiled for (rt_traits_kernel: rt_variant_traits of its shape) or 0, and RT_LOOP_CULL as whether the kernel reads the primary-ray cull's plane
 * (rt_render_kernel and rt_traits_kernel: rt_loop_culls of the shape and the kernel; false in the loops).  Text, not a function: called as a function the loop compiles to other code in all thirteen render
 * kernels, and the render kernel's code is kept byte for byte.
 */
{
    constexpr bool BUDGET = RT_LOOP_BUDGET;
    constexpr bool VIEWS = RT_LOOP_VIEWS;
    constexpr bool SKY = RT_LOOP_SKY;
    constexpr int TRAITS = RT_LOOP_TRAITS;      /* RT_TRAIT_* the scene is known to have (rt_traits_kernel; `a` is then an rt_traits_args), 0 everywhere else */
    constexpr bool CULL = RT_LOOP_CULL;         /* primary rays of pixels the view's cull plane flags skip the meshes (rt_cull.h) */
    constexpr bool ONE_MESH = HAS_MESH && (TRAITS & RT_TRAIT_ONE_MESH) != 0;
    static_assert(!CULL || ONE_MESH, "the cull acts where the ONE_MESH kernel tests its one root box: there is no form of it for the MESH section");
    extern __shared__ v4f lds_raw[];
    const int tid = threadIdx.x;
    const int lane = tid & (RT_WAVE - 1);

    Lds L;
    uint2 *stack;        /* [stack_entries + 1][NT] deferred sibling: (entry distance bits, reference) */
    if (MODE != RT_SCENE_GLOBAL) {
        /* stage the scene (or its part before the triangles) into LDS: coalesced 16-byte loads, one pass per workgroup */
        const int staged = MODE == RT_SCENE_LDS ? a.blob_f4 : a.off_tris;
        for (int i = tid; i < staged; i += NT) lds_raw[i] = ((const v4f *)a.blob)[i];
        L.nodes = lds_raw + a.off_nodes;
        L.objs = lds_raw + a.off_objlds;
        L.meshes = lds_raw + a.off_meshes;
        L.objtab = lds_raw + a.off_objtab;
        L.tris = MODE == RT_SCENE_LDS ? lds_raw + a.off_tris : (const v4f *)a.blob + a.off_tris;
        stack = (uint2 *)(lds_raw + staged);
    } else {
        const v4f *g = (const v4f *)a.blob;
        L.nodes = g + a.off_nodes;
        L.tris = g + a.off_tris;
        L.objs = g + a.off_objlds;
        L.meshes = g + a.off_meshes;
        L.objtab = g + a.off_objtab;
        stack = (uint2 *)lds_raw;
    }
    __syncthreads();
    uint2 *const my_stack = stack + tid;        /* this lane's column of the [entry][thread] stack */

    Frame f;
    frame_init(f, a);
    Px p;
    px_init(p);
    /* ---- per-lane traversal state (registers + LDS stack); a lane is traversing iff M_WAIT ---- */
    uint32_t cur = 0;
    int sp = 0, w_prim = -1;
    float w_best = RT_INF_F;
    /* this traversal's ray, one word: bit 0 - RT_RAY_ZERO_DIR - says that its direction has a component of exactly zero (box_enter rather than
     * box_enter_med3); an integer, so that its lane mask is one compare.  CULL: bits 1..31 are the traversal's dead gates (the subtree cull,
     * rt_cull.h) - the pixel's gate word for a primary ray, 0 for a bounce ray - so the flag is read through RT_ZERO_DIR_LANES() alone, which masks */
    uint32_t w_ray_bits = 0u;
    constexpr uint32_t RT_RAY_ZERO_DIR = 1u;
    static_assert((RT_RAY_ZERO_DIR & ~1u) == 0u, "gate g is bit g, g >= 1 (rt_device_scene.h): bit 0 is the zero-direction flag's");
    /* (a macro, not a lambda: through a lambda 35 kernels that are not compiled with CULL come out with other code) */
#define RT_ZERO_DIR_LANES() __builtin_amdgcn_uicmp(CULL ? w_ray_bits & RT_RAY_ZERO_DIR : w_ray_bits, 0u, RT_ICMP_NE)
    /* CULL: the pixel's gate word, loaded by px_fetch with the pixel's cull bit and held in this register between the pixel's samples (the
     * alternatives and what was measured: DESIGN.md section 24, "The subtree cull") */
    uint32_t px_gates = 0u;
    /* CULL: the word the mesh start acts on for the ray px_gen has just made: px_gates, or a table pixel's sub-word (rt_entry.h) */
    uint32_t start_word = 0u;
    Chunk ch;
    ch.next = 0; ch.end = 0; ch.frame = 0; ch.exhausted = false;
#ifdef RT_STATS
    unsigned st_exec[ST_N], st_lanes[ST_N];
    for (int i = 0; i < ST_N; i++) { st_exec[i] = 0; st_lanes[i] = 0; }
    unsigned long long st_time[TM_N], st_last = __builtin_readcyclecounter();
    const unsigned long long st_wall0 = wall_clock64();
    for (int i = 0; i < TM_N; i++) st_time[i] = 0;
#endif

    for (;;) {
        RT_STAT(ST_ITER);
        RT_LAP(TM_CTL);
        /* A ray that hit nothing costs a handful of instructions (sky, end of sample): it is
         * finished on the spot and the lane generates its next ray in this same round.  Hits
         * (several hundred instructions: three Box-Muller draws, four normalisations) are shaded
         * in batches: without a mesh the lanes holding one wait until `shade_batch` of them
         * do, or nobody else can move, while the others go on generating; with a mesh the
         * traversal loop below already yields in batches (`ready_break`).
         * Progress: whenever the traversal loop below leaves on a batch of hits with no cheap-work lane around, this
         * condition has to take the batch, or the wave comes back with nothing changed.  Both conditions are stated in
         * rt_device_scene.h (RT_ROUND_SHADES, rt_traversal_yields), where tests/sanitize/capi_host_fuzz.cpp (check_progress) takes
         * them from too. */
        if (p.mode == M_SHADE && p.best_obj < 0) px_shade_miss<BUDGET, VIEWS, SKY, CULL>(p, a, f);
        {
            const int n_hit = __popcll(__builtin_amdgcn_uicmp((unsigned)p.mode, (unsigned)M_SHADE, RT_ICMP_EQ));
            const bool others = (__builtin_amdgcn_uicmp((unsigned)p.mode, (unsigned)M_GEN, RT_ICMP_EQ) |
                                 (ch.exhausted ? 0ull : __builtin_amdgcn_uicmp((unsigned)p.mode, (unsigned)M_FETCH, RT_ICMP_EQ))) != 0ull;
            const int n_trav = __popcll(__builtin_amdgcn_uicmp((unsigned)p.mode, (unsigned)M_WAIT, RT_ICMP_EQ));
            if (RT_ROUND_SHADES(a, HAS_MESH, n_hit, n_trav, others)) {
                if (p.mode == M_SHADE) {
                    RT_STAT(ST_SHADE);
                    px_shade<!(NT == 1024 && HAS_MESH), MODE == RT_SCENE_HYBRID, BUDGET, VIEWS, (TRAITS & RT_TRAIT_PLAIN_MATERIALS) != 0, CULL>(p, a, f, L);
                }
            }
        }
        RT_LAP(TM_SHADE);
        if (CULL) px_fetch<BUDGET, VIEWS, CULL>(p, ch, a, f, lane, &px_gates);
        else px_fetch<BUDGET, VIEWS, CULL>(p, ch, a, f, lane);
        if (BUDGET) {
            /* Where budgets are sparse most slots hand their lane nothing.  A lane left in M_FETCH asks again at once instead of idling through
             * a round of the others' work: until every lane has a pixel to trace or the tiles are out (then px_fetch ends the lanes left).
             * The condition is a ballot, so the whole wave makes every call; each call uses up at least one slot per asking lane or sets
             * ch.exhausted, after which the calls hand out what is left of the chunk in hand and end every other asking lane - a tile whose 64
             * budgets are zero costs one pass. */
            while (__builtin_amdgcn_uicmp((unsigned)p.mode, (unsigned)M_FETCH, RT_ICMP_EQ) != 0ull) px_fetch<true>(p, ch, a, f, lane);
        }
        RT_LAP(TM_FETCH);
        if (p.mode == M_GEN) {
            RT_STAT(ST_GEN);
            if (CULL) px_gen<HAS_MESH, TRAITS, CULL>(p, a, L, &f, px_gates, &start_word);
            else px_gen<HAS_MESH, TRAITS>(p, a, L);
            if (ONE_MESH) {
                /* the one mesh's root box, tested here and once: the MESH section's trip below with next_mesh == 0, and none after it (the
                 * ray came out of px_gen as M_SHADE, which it stays unless it enters the box) */
                RT_STAT(ST_MESH);
                const v4f m0 = L.meshes[0], m1 = L.meshes[1];
                /* (CULL: a primary ray - bounce 0 - of a pixel the view's cull plane flags does not test the root box and stays M_SHADE: it would
                 * enter no leaf, rt_cull.h.  Nothing else about the ray changes: the same draws, the same simple-object hit, the same shade.
                 * So does a primary ray whose sub-word is `nothing`, RT_SUB_NOTHING in a table: no gate word and no tagged triangle reads so) */
                if (!(CULL && ((unsigned)p.bounce | (p.id & PX_NOCULL)) == 0u) && !(CULL && ((unsigned)p.bounce | (start_word ^ RT_SUB_NOTHING)) == 0u) && !(p.d.x != p.d.x || p.d.y != p.d.y || p.d.z != p.d.z)) {
                    const uint32_t root_ref = __float_as_uint(m1.z);
                    float rd;
                    const bool rh = box_test(m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, p.o, p.inv, rd);
                    if (!(!rh || rd > RT_INF_F || ((root_ref & RT_REF_CHAIN) && !(rd < RT_INF_F)))) {
                        cur = root_ref; sp = 0; w_best = RT_INF_F; w_prim = -1;
                        w_ray_bits = (p.d.x == 0.0f || p.d.y == 0.0f || p.d.z == 0.0f) ? RT_RAY_ZERO_DIR : 0u;
                        if (CULL) {
                            /* a primary ray of a pixel whose word is tagged `triangle T` (rt_entry.h) starts on the one-triangle leaf (T)
                             * with an empty stack and no gates: the leaf section tests T against best = RT_INF_F and merges.  Else the word
                             * is the pixel's gate word.  For a table pixel's primary ray px_gen has put the sub-box's word there: a tagged
                             * triangle, or the pixel's gate word where the sub-box is not known (rt_entry.h) */
                            const bool tagged = p.bounce == 0 && (start_word & RT_ENTRY_TAG) != 0u;
                            if (tagged) cur = rt_entry_leaf(start_word);
                            w_ray_bits |= p.bounce == 0 && !tagged ? start_word & ~RT_RAY_ZERO_DIR : 0u;
                        }
                        p.mode = M_WAIT;
                        p.frame_steps |= 0x80000000u;
                        RT_STAT(ST_MESH_START);
                    }
                }
            }
        }
        /* CULL: px_gen's load of a table pixel's sub-word is waited for here, on every path: a lane that does not reach the mesh start (a flagged
         * pixel, a NaN direction) would carry it into the traversal loops, where the compiler then puts a wait into the descend and the leaf
         * loop.  RT_WAIT_VMCNT0 (rt_pixel.h) is the gfx9 encoding of s_waitcnt vmcnt(0) with expcnt and lgkmcnt left alone.  It waits for every
         * vector load outstanding, not only that one: here, at the end of the generate section, px_gen's load is the only one there can be
         * (the section's other operands come from LDS and registers, and px_fetch's loads are consumed in px_fetch) */
        if (CULL) __builtin_amdgcn_s_waitcnt(RT_WAIT_VMCNT0);
        RT_LAP(TM_GEN);

        if (HAS_MESH) {
            /* ================= MESH: find the next mesh whose root box the ray enters ======= */
            while (!ONE_MESH && p.mode == M_MESH) {
                RT_STAT(ST_MESH);
                if (p.next_mesh >= a.num_meshes) { p.mode = M_SHADE; break; }
                const v4f m0 = L.meshes[2 * p.next_mesh], m1 = L.meshes[2 * p.next_mesh + 1];
                p.next_mesh++;
                /* a NaN direction (Box-Muller on a zero draw, SURVEY.md App. A.13) fails every
                 * triangle test: the mesh cannot be hit, no need to walk it */
                if (p.d.x != p.d.x || p.d.y != p.d.y || p.d.z != p.d.z) continue;
                /* the root is pushed unconditionally and tested when popped (src/objects.cu:494-501) */
                const uint32_t root_ref = __float_as_uint(m1.z);
                float rd;
                const bool rh = box_test(m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, p.o, p.inv, rd);
                if (!rh || rd > RT_INF_F || ((root_ref & RT_REF_CHAIN) && !(rd < RT_INF_F))) continue;
                cur = root_ref; sp = 0; w_best = RT_INF_F; w_prim = -1;
                w_ray_bits = (p.d.x == 0.0f || p.d.y == 0.0f || p.d.z == 0.0f) ? RT_RAY_ZERO_DIR : 0u;
                p.mode = M_WAIT;
                p.frame_steps |= 0x80000000u;           /* (cost bookkeeping: this pixel traverses) */
                RT_STAT(ST_MESH_START);
            }

            RT_LAP(TM_MESH);
            /* ================= WORK: BVH traversal steps (src/objects.cu:487-532, :586-600) ====
             * Runs while enough lanes are traversing; lanes whose ray is finished go back to
             * shading as soon as the traversing group is small.  Visit order, push order and
             * every comparison are the reference's. */
            const V3 o = p.o, d = p.d, inv = p.inv;
            for (;;) {
                /* the three lane counts from four compare masks combined in scalar registers (a __ballot of a bool built from
                 * several compares is rebuilt through a v_cndmask and a v_cmp) */
                const unsigned long long m_wait = __builtin_amdgcn_uicmp((unsigned)p.mode, (unsigned)M_WAIT, RT_ICMP_EQ);
                const int n_active = __popcll(m_wait);
                if (n_active == 0) break;
                /* lanes holding a hit wait for a batch of `hit_break`; the cheap kinds of ready
                 * lane (generate, fetch, next mesh, a miss) for one of `ready_break` */
                const unsigned long long m_hit = __builtin_amdgcn_uicmp((unsigned)p.mode, (unsigned)M_SHADE, RT_ICMP_EQ) & __builtin_amdgcn_sicmp(p.best_obj, 0, RT_ICMP_SGE);
                const unsigned long long m_done = __builtin_amdgcn_uicmp((unsigned)p.mode, (unsigned)M_DONE, RT_ICMP_EQ);
                const int n_hit = __popcll(m_hit);
                const int n_light = __popcll(__ballot(1) & ~(m_wait | m_done | m_hit));
                /* ... or a smaller batch of hits that, together with the cheap-work lanes, is worth the round: where
                 * every traversal ends in a hit (a closed scene) hits fill a big batch fast and big batches are what
                 * the 700-instruction shade wants; where most rays escape (an open scene) hits are rare, the lanes
                 * holding one would idle for long, and the round is paid for by the escaped lanes anyway */
                if (rt_traversal_yields(a, n_hit, n_active, n_light)) break;
#if defined(RT_COSTMAP) && RT_COSTMAP == 2
                p.c_wsteps += 1;      /* wave-level macro steps this lane lived through */
#endif
                RT_LAP(TM_CTL);
                if (p.mode == M_WAIT) {
                    RT_STAT(ST_WORK_ITER);
                    p.frame_steps += (unsigned)(RT_COST_STEP * RT_MAX_BATCH_FRAMES);   /* one more traversal macro step (the bits above the frame index) */
                    /* one macro step: descend to a leaf (or run out of children), test the
                     * leaf's triangles, pop the next deferred sibling.  The lane's whole
                     * traversal state is `cur` (+ the stack): an internal node to descend from,
                     * or a leaf whose triangles are tested and after which the stack is popped;
                     * "no child entered" is the empty leaf. */
                    /* two copies of the loop: the six-med3 slab test where no traversing ray of the wave has a direction
                     * component of exactly zero (always, in practice), the reference's min / max form otherwise */
                    if (rt_descend_pops(NT, MODE)) {
                        /* the loop pops behind a dead end and goes on (rt_descend_pop, rt_traverse.h): what it hands the leaf section
                         * is a leaf with triangles, a finished mesh, or what the descend_keep rule sent out early */
                        if (rt_descend_pop_enters(cur, sp)) {
                            if (RT_ZERO_DIR_LANES() == 0ull) rt_descend_pop<NT, true, CULL>(cur, sp, my_stack, L, o, inv, w_best, a.descend_keep, w_ray_bits RT_STAT_ARGS);
                            else rt_descend_pop<NT, false, CULL>(cur, sp, my_stack, L, o, inv, w_best, a.descend_keep, w_ray_bits RT_STAT_ARGS);
                        }
                    } else if (!(cur & RT_REF_LEAF)) {
                        if (RT_ZERO_DIR_LANES() == 0ull) rt_descend<NT, true>(cur, sp, my_stack, L, o, inv, w_best, a.descend_keep RT_STAT_ARGS);
                        else rt_descend<NT, false>(cur, sp, my_stack, L, o, inv, w_best, a.descend_keep RT_STAT_ARGS);
                    }
                    RT_LAP_SPLIT(TM_DESCEND)
                    if (cur & RT_REF_LEAF) {
                        /* leaf: strict <, first triangle wins ties (:596) */
                        const int start = (int)(cur & RT_REF_START_MASK);
                        const int count = (int)((cur >> RT_REF_COUNT_SHIFT) & RT_REF_COUNT_MAX);
                        for (int k = 0; k < count; k++) {
                            RT_STAT(ST_LEAF_TRI);
                            RT_COST(p.c_steps++);
                            float t;
                            const unsigned long long closer = tri_closer_lanes(L.tris, start + k, o, d, w_best, t);
                            w_best = rt_sel_f32(closer, t, w_best);
                            w_prim = (int)rt_sel_u32(closer, (uint32_t)(start + k), (uint32_t)w_prim);
                        }
                        RT_LAP_SPLIT_LEAF(TM_LEAF)
                        /* pop one entry: it is taken iff !(dist > best) (:501); through a
                         * collapsed chain iff dist < best (:517) - the distance is never NaN, so
                         * that is dist < best, or dist == best on a plain edge.  A lane whose entry
                         * is refused stays on the empty leaf and pops again next step (rare). */
                        if (sp > 0) {
                            RT_STAT(ST_POP);
                            cur = rt_pop<NT>(sp, my_stack, w_best);
                        } else {
                            RT_STAT(ST_DONE_MESH);
                            /* this mesh is done: merge (smaller distance, or equal and later in the list);
                             * its place in the object list is read again here rather than kept in a register */
                            const int w_obj = ONE_MESH ? px_traits(a).mesh_obj : (int)__float_as_uint(L.meshes[2 * (p.next_mesh - 1) + 1].w);
                            if (w_prim >= 0 && (w_best < p.best_t || (w_best == p.best_t && w_obj > p.best_obj))) {
                                p.best_t = w_best; p.best_obj = w_obj; p.best_prim = w_prim;
                            }
                            p.mode = ONE_MESH || p.next_mesh >= a.num_meshes ? M_SHADE : M_MESH;
                        }
                    }
                }
                RT_LAP(TM_POP);
            }
        }

        if (__ballot(p.mode != M_DONE) == 0ull) break;
    }
#undef RT_ZERO_DIR_LANES
    RT_STATS_FLUSH();
}
