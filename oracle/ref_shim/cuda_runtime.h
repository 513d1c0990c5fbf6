/*
 * Stand-in for <cuda_runtime.h>: just enough for the reference's kernel source to compile as host C++
 * and be driven one "thread" at a time by oracle/ref_driver.cpp.  TEST INFRASTRUCTURE ONLY, our own text.
 *
 *   __global__ / __device__ / __host__   nothing
 *   __shared__                           static: one table per process, primed once by the driver
 *   threadIdx, blockIdx, blockDim, gridDim   thread_local index structs the driver sets before each call
 *   __syncthreads()                      no-op (the driver primes the static tables before the first ray)
 *   atomicAdd(double *, double)          a plain add (an "omp atomic" add when the driver runs several
 *                                        host threads) that also counts its calls: ray-steps = calls / 8
 */
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __shared__ static

struct ref_shim_dim3 {
    unsigned x, y, z;
};
inline thread_local ref_shim_dim3 threadIdx = {0, 0, 0}, blockIdx = {0, 0, 0}, blockDim = {1, 1, 1},
                                  gridDim = {1, 1, 1};
inline thread_local unsigned long long ref_shim_atomic_calls = 0;
inline bool ref_shim_concurrent = false;      /* set once by the driver before any ray is traced */

typedef int cudaError_t;

inline void __syncthreads() {}

inline double atomicAdd(double *address, double value) {
    ++ref_shim_atomic_calls;
    if (!ref_shim_concurrent) {
        *address += value;
    } else {
#pragma omp atomic
        *address += value;
    }
    return 0.0; /* the kernel source never uses the old value */
}
