/*
 * rt_cull_kernel.h — the primary-ray cull's pre-pass (rt_cull.h): a streaming kernel, one thread per pixel of the full image, that walks
 * every mesh's nodes in global memory with the predicate and writes one bit per pixel, 32 pixels to a word, and behind the bits one word
 * per pixel: the subtree cull's dead gates (rt_cull_gate_word).  Once per view (rt_capi.cpp keeps the plane); nothing of the wave loop, plain HIP.
 */
#ifndef RT_CULL_KERNEL_H
#define RT_CULL_KERNEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_cull.h"
#include "rt_device_scene.h"
#include "rt_entry.h"
#include "rt_launch.h"

#define RT_CULL_THREADS 256

struct rt_cull_args {
    float cam[12];
    int32_t width, height, antialias;
    int32_t gates;               /* 0: every gate word is written as 0 (RT_AMD_SUBTREE_CULL=0, or a scene of several meshes: the words are one mesh's) */
    int32_t entry;               /* 0: every entry word is written as 0 (RT_AMD_PRIMARY_ENTRY=0, or a scene of several meshes) */
    int32_t off_tris, num_tris;  /* the triangles the entry words are about: where they start in the blob, and how many the nodes' leaves may name */
    const float *blob;
    int32_t off_nodes, num_nodes, off_meshes, num_meshes;
    uint32_t *plane;             /* rt_cull_alloc_words_entry(rt_cull_words(width, height)) words: the bits, then a gate word and then an entry word per thread of the grid */
};

/* a thread's column of the walk's stack in LDS, [entry][thread] */
struct rt_cull_lds_stack {
    uint32_t *column;
    __device__ uint32_t &operator[](int i) { return column[i * RT_CULL_THREADS]; }
};

/* Thread i has pixel i (py * width + px); a wave's 64 answers are one ballot, whose halves lanes 0 and 32 store: whole words, no atomics.
 * The grid covers rt_cull_words * 32 pixels, so every word of the plane is written; a thread past the image answers 0.  Every thread then
 * writes its gate word (0 past the image and without `gates`; a flagged pixel has every gate dead) and its entry word (rt_entry.h; 0 past
 * the image, without `entry` and for a flagged pixel). */
__global__ __launch_bounds__(RT_CULL_THREADS) void rt_cull_kernel(const rt_cull_args a)
{
    __shared__ uint32_t stacks[RT_CULL_STACK * RT_CULL_THREADS];
    __shared__ uint32_t bounds[RT_CULL_STACK * RT_CULL_THREADS];       /* the entry walk's path bounds, beside its pending references */
    const size_t i = (size_t)blockIdx.x * RT_CULL_THREADS + threadIdx.x;
    const size_t pixels = (size_t)a.width * (size_t)a.height;
    bool flagged = false;
    uint32_t gate_word = 0u, entry_word = 0u;
    if (i < pixels) {
        const int py = (int)(i / (size_t)a.width), px = (int)(i - (size_t)py * (size_t)a.width);
        float P[3];
        rt_cull_primary(a.cam, px, py, P);
        const rt_cull_cone c = rt_cull_cone_of(P, a.cam, a.antialias);
        flagged = rt_cull_no_leaf(c, a.blob, a.off_nodes, a.num_nodes, a.off_meshes, a.num_meshes, rt_cull_lds_stack{stacks + threadIdx.x});
        if (a.gates) gate_word = rt_cull_gate_word(c, a.blob, a.off_nodes, a.num_nodes, a.off_meshes, 0, rt_cull_lds_stack{stacks + threadIdx.x});
        if (a.entry && !flagged)
            entry_word = rt_entry_word(c, a.blob, a.off_nodes, a.num_nodes, a.off_meshes, 0, a.off_tris, a.num_tris, rt_cull_lds_stack{stacks + threadIdx.x}, rt_cull_lds_stack{bounds + threadIdx.x});
    }
    const unsigned long long bits = __ballot(flagged);
    const int lane = threadIdx.x & 63;
    const size_t word = i >> 5;
    if (word < rt_cull_words(a.width, a.height)) {
        if (lane == 0) a.plane[word] = (uint32_t)bits;
        if (lane == 32) a.plane[word] = (uint32_t)(bits >> 32);
        a.plane[rt_cull_words(a.width, a.height) + i] = gate_word;
        a.plane[rt_cull_entry_base(rt_cull_words(a.width, a.height)) + i] = entry_word;
    }
}

/* ---- the refinement (rt_entry.h, "The sub-entry words"): two kernels behind the pre-pass, or on their own over a plane that has its view's
 * words.  rt_sub_compact_kernel, one thread per pixel, hands every unflagged pixel whose entry word is 0 a slot from the counter (zeroed by
 * the launcher), writes the slot into the pixel's entry word and the pixel into the slot's word; a pixel that finds the tables full keeps
 * 0.  rt_sub_refine_kernel then runs one thread per (slot, sub-box): the 64 lanes of a wave walk the 64 sub-cones of one pixel, which are
 * neighbours, so a wave is evenly loaded whatever the image looks like.  Every word of every table in use is written.  The number of tables in
 * use is known on the device only, so the grid is the image's bound, cap x 64 threads (16.6 M, 64,800 workgroups at 1080p, where the monkey
 * uses 47 % of them): a workgroup past the counter reads it and ends, which is part of the 14.5 ms measured there; nothing was tuned. */
__global__ __launch_bounds__(RT_CULL_THREADS) void rt_sub_compact_kernel(const rt_cull_args a)
{
    const size_t i = (size_t)blockIdx.x * RT_CULL_THREADS + threadIdx.x;
    const size_t pixels = (size_t)a.width * (size_t)a.height, words = rt_cull_words(a.width, a.height);
    if (i >= pixels) return;
    uint32_t *const entry = a.plane + rt_cull_entry_base(words) + i;
    const bool flagged = ((a.plane[i >> 5] >> (i & 31u)) & 1u) != 0u;
    if (!rt_sub_wants_table(flagged, *entry)) return;
    const uint32_t slot = atomicAdd(a.plane + rt_sub_header_base(words), 1u);
    if ((size_t)slot < rt_sub_cap(words)) {
        a.plane[rt_sub_pixels_base(words) + slot] = (uint32_t)i;
        *entry = rt_sub_slot_word(slot);
    } else {
        *entry = 0u;
    }
}

__global__ __launch_bounds__(RT_CULL_THREADS) void rt_sub_refine_kernel(const rt_cull_args a)
{
    __shared__ uint32_t stacks[RT_CULL_STACK * RT_CULL_THREADS];
    __shared__ uint32_t bounds[RT_CULL_STACK * RT_CULL_THREADS];
    const size_t t = (size_t)blockIdx.x * RT_CULL_THREADS + threadIdx.x;
    const size_t words = rt_cull_words(a.width, a.height), cap = rt_sub_cap(words), slot = t / RT_SUB_WORDS;
    const uint32_t idx = (uint32_t)(t % RT_SUB_WORDS);
    const size_t handed = a.plane[rt_sub_header_base(words)];        /* (the counter runs past cap where the tables are full) */
    if (slot >= cap || slot >= handed) return;
    const size_t i = a.plane[rt_sub_pixels_base(words) + slot];
    uint32_t word = 0u;
    if (i < (size_t)a.width * (size_t)a.height) {
        const int py = (int)(i / (size_t)a.width), px = (int)(i - (size_t)py * (size_t)a.width);
        float P[3];
        rt_cull_primary(a.cam, px, py, P);
        const rt_cull_cone c = rt_sub_cone_of(P, a.cam, idx);
        word = rt_entry_word(c, a.blob, a.off_nodes, a.num_nodes, a.off_meshes, 0, a.off_tris, a.num_tris, rt_cull_lds_stack{stacks + threadIdx.x}, rt_cull_lds_stack{bounds + threadIdx.x});
    }
    /* (stored with the pixel's gate word where it is not known: rt_entry.h, "What a table stores") */
    a.plane[rt_sub_tables_base(words) + slot * RT_SUB_WORDS + idx] = rt_sub_stored(word, i < (size_t)a.width * (size_t)a.height ? a.plane[words + i] : 0u);
}

extern "C" hipError_t rt_launch_cull(const float *cam, int32_t width, int32_t height, int32_t view_flags, const rt_f4 *blob, int32_t off_nodes, int32_t num_nodes,
                                     int32_t off_meshes, int32_t num_meshes, uint32_t *plane, hipStream_t stream)
{
    if (!cam || !blob || !plane || width <= 0 || height <= 0 || num_nodes < 0 || num_meshes < 0) return hipErrorInvalidValue;
    rt_cull_args a;
    for (int k = 0; k < 12; k++) a.cam[k] = cam[k];
    a.width = width; a.height = height; a.antialias = (view_flags & RT_CULL_ANTIALIAS) ? 1 : 0;
    a.gates = (view_flags & RT_CULL_WITH_GATES) && num_meshes == 1 ? 1 : 0;
    a.entry = (view_flags & RT_CULL_WITH_ENTRY) && num_meshes == 1 ? 1 : 0;
    a.off_tris = (int32_t)((uint32_t)view_flags >> RT_CULL_TRIS_SHIFT);
    a.num_tris = (int32_t)(RT_REF_START_MASK + 1u);      /* (a leaf names at most that many; the blob ends with the triangles its leaves name) */
    a.blob = (const float *)blob;
    a.off_nodes = off_nodes; a.num_nodes = num_nodes; a.off_meshes = off_meshes; a.num_meshes = num_meshes;
    a.plane = plane;
    const size_t words = rt_cull_words(width, height), threads = words * 32;
    const size_t sub_blocks = (rt_sub_cap(words) * RT_SUB_WORDS + RT_CULL_THREADS - 1) / RT_CULL_THREADS;
    if (threads / RT_CULL_THREADS + 1 > 0x7fffffffu || sub_blocks > 0x7fffffffu) return hipErrorInvalidValue;      /* (an image beyond check_image_size's 2^28 pixels) */
    const unsigned blocks = (unsigned)((threads + RT_CULL_THREADS - 1) / RT_CULL_THREADS);
    /* RT_CULL_WITH_SUBENTRY alone: the plane has this view's words, only the refinement is queued (the view's first reuse, rt_cull_host::Plan) */
    const bool refine = (view_flags & RT_CULL_WITH_SUBENTRY) && a.antialias && num_meshes == 1, refine_only = refine && !(view_flags & RT_CULL_WITH_ENTRY);
    if (!refine_only) hipLaunchKernelGGL(rt_cull_kernel, dim3(blocks), dim3(RT_CULL_THREADS), 0, stream, a);
    if (refine) {
        /* (the plane then has rt_sub_alloc_words(words) words: the caller's side of the flag) */
        hipError_t e = hipMemsetAsync(plane + rt_sub_header_base(words), 0, RT_SUB_HEADER * 4, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(rt_sub_compact_kernel, dim3(blocks), dim3(RT_CULL_THREADS), 0, stream, a);
        hipLaunchKernelGGL(rt_sub_refine_kernel, dim3((unsigned)sub_blocks), dim3(RT_CULL_THREADS), 0, stream, a);
    }
    return hipGetLastError();
}

#endif
