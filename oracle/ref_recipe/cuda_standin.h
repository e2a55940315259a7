/*
 * cuda_standin.h — the few CUDA names the reference renderer uses, as plain host C++ (TEST
 * INFRASTRUCTURE).  With it the reference's own sources compile and run on the CPU; see
 * oracle/ref_build.py.  Written from the CUDA runtime API's public names; it holds nothing of
 * the reference.
 */
#ifndef RT_REF_CUDA_STANDIN_H
#define RT_REF_CUDA_STANDIN_H

/* <math.h>, not <cmath> alone: it puts the float overloads of sqrt/log/cos/... into the global
 * namespace, so log(float) resolves to the float function as it does under nvcc. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <sys/types.h>      /* uint */
#include <string>

#define __host__
#define __device__
#define __global__
#define __constant__

typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };

static inline cudaError_t cudaMalloc(void **p, size_t n) { *p = malloc(n ? n : 1); return *p ? cudaSuccess : 2; }
template <typename T> static inline cudaError_t cudaMallocManaged(T **p, size_t n) { return cudaMalloc((void **)p, n); }
static inline cudaError_t cudaFree(void *p) { free(p); return cudaSuccess; }
static inline cudaError_t cudaMemcpy(void *dst, const void *src, size_t n, cudaMemcpyKind) { if (n) memcpy(dst, src, n); return cudaSuccess; }
template <typename T> static inline cudaError_t cudaMemcpyToSymbol(T &symbol, const void *src, size_t n) { memcpy((void *)&symbol, src, n); return cudaSuccess; }
static inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
static inline cudaError_t cudaPeekAtLastError() { return cudaSuccess; }
static inline const char *cudaGetErrorString(cudaError_t e) { return e == cudaSuccess ? "no error" : "out of memory"; }

struct float3 { float x, y, z; };
struct uint3 { unsigned int x, y, z; };
struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int vx = 1, unsigned int vy = 1, unsigned int vz = 1) : x(vx), y(vy), z(vz) {}
};

extern thread_local uint3 threadIdx, blockIdx;
extern thread_local dim3 blockDim, gridDim;

/* CUDA's global min/max overload set: float pairs are fminf/fmaxf (a NaN operand is dropped), a
 * mixed float/double pair is promoted to double. */
static inline float min(float a, float b) { return fminf(a, b); }
static inline float max(float a, float b) { return fmaxf(a, b); }
static inline double min(double a, double b) { return fmin(a, b); }
static inline double max(double a, double b) { return fmax(a, b); }
static inline double min(float a, double b) { return fmin((double)a, b); }
static inline double max(float a, double b) { return fmax((double)a, b); }
static inline double min(double a, float b) { return fmin(a, (double)b); }
static inline double max(double a, float b) { return fmax(a, (double)b); }
static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }

#endif
