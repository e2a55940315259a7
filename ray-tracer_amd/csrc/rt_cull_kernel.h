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
    const size_t threads = rt_cull_words(width, height) * 32;
    hipLaunchKernelGGL(rt_cull_kernel, dim3((unsigned)((threads + RT_CULL_THREADS - 1) / RT_CULL_THREADS)), dim3(RT_CULL_THREADS), 0, stream, a);
    return hipGetLastError();
}

#endif
