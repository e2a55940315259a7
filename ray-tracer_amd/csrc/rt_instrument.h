/*
 * rt_instrument.h — the development instrumentation of the render kernel (-DRT_STATS, -DRT_COSTMAP, -DRT_MARK): macros only, all of them
 * empty in the product.  They name the variables of the code they are placed in (lane, st_exec, st_lanes, st_time, st_last, p, cur, a), and
 * RT_LAP_SPLIT / RT_LAP_SPLIT_LEAF close and reopen the braces around them: read them beside rt_render_kernel.h, where they are used.
 */
#ifndef RT_INSTRUMENT_H
#define RT_INSTRUMENT_H

/* Development instrumentation (-DRT_STATS, tools/stats_run.py): per code section, how many
 * times a wave executed it and with how many active lanes.  Compiled out of the product. */
#ifdef RT_STATS
#define RT_STAT(slot) do { unsigned long long m_ = __ballot(1); if (lane == __builtin_ctzll(m_)) { st_exec[slot] += 1u; st_lanes[slot] += (unsigned)__popcll(m_); } } while (0)
#else
#define RT_STAT(slot) do { } while (0)
#endif
/* ... and (lap timer, s_memtime) where a wave's time goes: RT_LAP(slot) charges the time since the
 * previous lap to `slot` */
enum { TM_CTL = 0, TM_SHADE = 1, TM_FETCH = 2, TM_GEN = 3, TM_MESH = 4, TM_DESCEND = 5, TM_LEAF = 6, TM_POP = 7, TM_N = 8 };
#ifdef RT_STATS
#define RT_LAP(slot) do { unsigned long long now_ = __builtin_readcyclecounter(); st_time[slot] += now_ - st_last; st_last = now_; } while (0)
/* inside the divergent `if (w_active)` block: leave it, lap with every lane, enter it again (the
 * timers are per-lane registers; only laps that all lanes execute measure the wave) */
#define RT_LAP_SPLIT(slot) } RT_LAP(slot); if (p.mode == M_WAIT) {
#define RT_LAP_SPLIT_LEAF(slot) } } RT_LAP(slot); if (p.mode == M_WAIT) { if (cur & RT_REF_LEAF) {
#elif defined(RT_MARK)
/* (tools/isa_sections.py: section boundaries as comments in the assembly) */
#define RT_LAP(slot) asm volatile("; LAP " #slot)
#define RT_LAP_SPLIT(slot) asm volatile("; LAP " #slot);
#define RT_LAP_SPLIT_LEAF(slot) asm volatile("; LAP " #slot);
#else
#define RT_LAP(slot) do { } while (0)
#define RT_LAP_SPLIT(slot)
#define RT_LAP_SPLIT_LEAF(slot)
#endif
enum { ST_ITER = 0, ST_SHADE = 1, ST_SHADE_HIT = 2, ST_FETCH = 3, ST_GEN = 4, ST_MESH = 5, ST_MESH_START = 6, ST_WORK_ITER = 7, ST_NODE = 8, ST_LEAF_TRI = 9, ST_POP = 10, ST_DONE_MESH = 11,
       ST_POP_LOOP = 12 /* pops inside rt_descend_pop (rt_traverse.h); ST_POP counts the post-leaf ones */, ST_N = 13 };
#define RT_STATS_TIME_BASE (2 * ST_N)   /* the counters' (wave executions, lanes) pairs come first, then TM_N lap times, the summed wave lifetimes and the wave count: tools/stats_run.py reads them by position */

/* -DRT_COSTMAP (tools/costmap.py): the frame holds per-pixel step counts and clock ticks instead of colours (Px, rt_pixel.h) */
#ifdef RT_COSTMAP
#define RT_COST(x) do { x; } while (0)
#else
#define RT_COST(x) do { } while (0)
#endif

/* what rt_descend (rt_traverse.h), which the render kernel shares with the ray kernels, takes for the counters above: the statistics' arrays,
 * or the cost map's step counter of the pixel (Px::c_steps) */
#if defined(RT_STATS)
#define RT_STAT_PARAMS , unsigned *st_exec, unsigned *st_lanes, int lane
#define RT_STAT_ARGS , st_exec, st_lanes, lane
#elif defined(RT_COSTMAP)
#define RT_STAT_PARAMS , unsigned &c_steps
#define RT_STAT_ARGS , p.c_steps
#else
#define RT_STAT_PARAMS
#define RT_STAT_ARGS
#endif
#ifdef RT_STATS
#define RT_STATS_FLUSH() do {                                                                              \
    for (int i = 0; i < ST_N; i++) {                                                                          \
        if (st_exec[i]) { atomicAdd(&a.stats[2 * i], (unsigned long long)st_exec[i]); atomicAdd(&a.stats[2 * i + 1], (unsigned long long)st_lanes[i]); } \
    }                                                                                                         \
    RT_LAP(TM_CTL);                                                                                           \
    if (lane == 0) {                                                                                          \
        for (int i = 0; i < TM_N; i++) atomicAdd(&a.stats[RT_STATS_TIME_BASE + i], st_time[i]);                               \
        atomicAdd(&a.stats[RT_STATS_TIME_BASE + TM_N], wall_clock64() - st_wall0);      /* summed wave lifetimes, 100 MHz ticks */ \
        atomicAdd(&a.stats[RT_STATS_TIME_BASE + TM_N + 1], 1ull);                        /* waves */                          \
    }                                                                                                         \
} while (0)
#else
#define RT_STATS_FLUSH() do { } while (0)
#endif

#endif
