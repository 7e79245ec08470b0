// Device helpers shared by the weighted bags (wbag.hip) and the weighted FM-pooled lookup (wfm.hip): the vector types of
// their kernels, the launch constants, the bag of an occurrence and the masked keys of the one-call applies.
#pragma once
#include "gather_dev.h"
#include "plan_dev.h"

namespace ha {

template <int VEC>
struct WVec;
template <>
struct WVec<1> {
    typedef float T;
    static __device__ __forceinline__ float get(const T &v, int) { return v; }
    static __device__ __forceinline__ void set(T &v, int, float x) { v = x; }
};
template <>
struct WVec<2> {
    typedef float T __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ float get(const T &v, int k) { return v[k]; }
    static __device__ __forceinline__ void set(T &v, int k, float x) { v[k] = x; }
};
template <>
struct WVec<4> {
    typedef float4v T;
    static __device__ __forceinline__ float get(const T &v, int k) { return v[k]; }
    static __device__ __forceinline__ void set(T &v, int k, float x) { v[k] = x; }
};

constexpr int kWbagWaves = 4;         // waves per workgroup of the forward and of the short-run apply
constexpr int kWbagLongWaves = 16;
constexpr int kWbagCoopPerWave = 8;   // occurrences per wave and round of the cooperative path
constexpr int kWbagCoopRound = (kWbagLongWaves - 1) * kWbagCoopPerWave;      // wave 0 runs the chain only
constexpr int kWbagLongBlocks = 256;  // workgroups that loop over the (long key, slice) items: one per compute unit

// ---- masked keys of the one-call apply --------------------------------------------------------------------------------------
// keys[i] = the row number of a live occurrence, `dead` (>= rows) for a dead one.
template <typename IdT>
__global__ __launch_bounds__(256) void wbag_mask_kernel(const IdT *__restrict__ ids, const float *__restrict__ weights, int64_t n,
                                                        uint64_t rows, uint64_t dead, uint64_t *__restrict__ keys) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t r = id_to_row<IdT>(ids[i]);
    keys[i] = (r < rows && weights[i] != 0.f) ? r : dead;
}

template <bool FIXED>
__device__ __forceinline__ int wbag_bag(int i, int bag, const int32_t *__restrict__ bag_of) {
    return FIXED ? i / bag : bag_of[i];
}

}  // namespace ha
