// Sparse optimizers and sparse L2 on indexed slices: AddL2RegularizationSparse,
// Momentum (plain and Nesterov), AdaGrad, Adam, AdamW, Lamb.
//
// Reference: src/ops/OptimizersSparse.cu -- add_l2_regularization_sparse :3-51, momentum / nesterov
// :101-231, adagrad_sparse_update :331-389, adam_sparse_update :391-455, adamw_sparse_update :457-522,
// Lamb :524-722; declarations src/common/c_runtime_api.h:639-700.  There every kernel is one thread per
// element with a 64-bit divide per element and, where ids may repeat (SGD, Momentum), float atomics.
// The callers deduplicate before AdaGrad / Adam / AdamW / Lamb / L2 (python/hetu/gpu_links/
// OptimizerLink.py:15,60,78,95,111) and do NOT before Momentum (:37-49).
//
// Here: ONE WAVE PER ROW.  The row id is wave-uniform (one scalar load), every lane moves 16-byte
// vectors of the gradient row and of the parameter / state rows it addresses (two vectors per lane per
// trip, all loads of a trip issued before the arithmetic), so a 2 KiB row is two 1-KiB wave
// instructions per array and nothing is divided.  Rows are unique for the deduplicated ops, so the
// read-modify-write needs no atomics; Momentum, whose ids repeat, goes through the index plan and the
// occurrence-ordered apply of scatter.hip (deterministic: the reference's atomics pick an arbitrary
// order).  Arithmetic keeps the reference's expression order (library built with -ffp-contract=off) and
// Lamb's two norms are accumulated in double, in a fixed order: every symbol here equals the float32 numpy
// restatement of oracle/cpu.py BIT FOR BIT on the MI355X (tests/test_gpu_optim_paths.py asserts it call by
// call, at every branch below), and that restatement is within 1.9 - 4.1 units of 2^-24 x (sum of |terms|)
// of a float64 evaluation (tests/test_optim_oracle.py).  The reference's own tests ask for 1e-5
// (tests/test_optimizer.py:117-300).  Arrays need not be 16-byte aligned (scalar paths); ids beyond the
// table are skipped.
#include "optim_dev.h"

namespace ha {

// capi.hip
int scratch_get(hipStream_t stream, size_t bytes, void **out);

template <int KIND>
struct Uses {
    static constexpr bool s1 = KIND == kAdaGrad || KIND == kAdam || KIND == kAdamW || KIND == kLambUpdate;
    static constexpr bool s2 = KIND == kAdam || KIND == kAdamW || KIND == kLambUpdate;
    static constexpr bool grad_in = KIND != kLambStep;
    static constexpr bool grad_out = KIND == kL2;
    static constexpr bool param_out = KIND != kL2 && KIND != kLambUpdate;
    static constexpr bool upd_in = KIND == kLambStep;
    static constexpr bool upd_out = KIND == kLambUpdate;
};

// VEC = 4: width % 4 == 0 and 16-byte aligned arrays; VEC = 1: anything else.
template <int KIND, int VEC>
__global__ __launch_bounds__(256) void sparse_row_kernel(float *__restrict__ param, uint64_t rows,
                                                         const float *__restrict__ ids,
                                                         float *__restrict__ grads, int n, int width,
                                                         float *__restrict__ s1, float *__restrict__ s2,
                                                         OptArgs a) {
    typedef Uses<KIND> U;
    const int lane = lane_id();
    const int wave = static_cast<int>(blockIdx.x) * 4 + static_cast<int>(threadIdx.x >> 6);
    const int nwaves = static_cast<int>(gridDim.x) * 4;
    float ratio = 0.f;
    if (KIND == kLambStep)   // norm2(param) / norm2(update), both over the indexed rows (:577)
        ratio = static_cast<float>(sqrt(a.norms[0])) / static_cast<float>(sqrt(a.norms[1]));
    for (int i = wave; i < n; i += nwaves) {
        const uint64_t r = static_cast<uint64_t>(f32_to_key(ids[i]));
        double sp = 0.0, su = 0.0;
        if (r < rows) {   // wave-uniform
            const uint64_t prow = r * static_cast<uint64_t>(width);
            const uint64_t grow = static_cast<uint64_t>(i) * static_cast<uint64_t>(width);
            for (int c0 = 0; c0 < width; c0 += 2 * kWave * VEC) {
                float p[2][VEC], g[2][VEC], x1[2][VEC], x2[2][VEC], up[2][VEC];
                int col[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    col[t] = c0 + (t * kWave + lane) * VEC;
                    const int lc = col[t] < width ? col[t] : 0;   // branch-free loads
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        g[t][k] = 0.f, x1[t][k] = 0.f, x2[t][k] = 0.f, up[t][k] = 0.f;
                    }
                    if (VEC == 4) {
                        *reinterpret_cast<float4v *>(p[t]) = ld4(param + prow + lc);
                        if (U::grad_in)
                            *reinterpret_cast<float4v *>(g[t]) = ld4(grads + grow + lc);
                        if (U::s1)
                            *reinterpret_cast<float4v *>(x1[t]) = ld4(s1 + prow + lc);
                        if (U::s2)
                            *reinterpret_cast<float4v *>(x2[t]) = ld4(s2 + prow + lc);
                        if (U::upd_in)
                            *reinterpret_cast<float4v *>(up[t]) = ld4(a.update + grow + lc);
                    } else {
                        p[t][0] = param[prow + lc];
                        if (U::grad_in)
                            g[t][0] = grads[grow + lc];
                        if (U::s1)
                            x1[t][0] = s1[prow + lc];
                        if (U::s2)
                            x2[t][0] = s2[prow + lc];
                        if (U::upd_in)
                            up[t][0] = a.update[grow + lc];
                    }
                }
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    if (col[t] >= width)
                        continue;
#pragma unroll
                    for (int k = 0; k < VEC; ++k)
                        opt_step<KIND>(p[t][k], g[t][k], x1[t][k], x2[t][k], a, up[t][k], sp, su, ratio);
                    if (VEC == 4) {
                        if (U::param_out)
                            st4(param + prow + col[t], *reinterpret_cast<float4v *>(p[t]));
                        if (U::grad_out)
                            st4(grads + grow + col[t], *reinterpret_cast<float4v *>(g[t]));
                        if (U::s1)
                            st4(s1 + prow + col[t], *reinterpret_cast<float4v *>(x1[t]));
                        if (U::s2)
                            st4(s2 + prow + col[t], *reinterpret_cast<float4v *>(x2[t]));
                        if (U::upd_out)
                            st4(a.update + grow + col[t], *reinterpret_cast<float4v *>(up[t]));
                    } else {
                        if (U::param_out)
                            param[prow + col[t]] = p[t][0];
                        if (U::grad_out)
                            grads[grow + col[t]] = g[t][0];
                        if (U::s1)
                            s1[prow + col[t]] = x1[t][0];
                        if (U::s2)
                            s2[prow + col[t]] = x2[t][0];
                        if (U::upd_out)
                            a.update[grow + col[t]] = up[t][0];
                    }
                }
            }
        }
        if (KIND == kLambUpdate) {   // this row's share of the two norms, fixed lane order
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                sp += __shfl_xor(sp, o, kWave);
                su += __shfl_xor(su, o, kWave);
            }
            if (lane == 0) {
                a.part_param[i] = sp;
                a.part_update[i] = su;
            }
        }
    }
}

// Lamb: sums of the per-row partials in a fixed order (one workgroup; n is a batch's unique count).
__global__ __launch_bounds__(1024) void lamb_norms_kernel(const double *__restrict__ pp,
                                                          const double *__restrict__ pu, int n,
                                                          double *__restrict__ norms) {
    __shared__ double s_p[16], s_u[16];
    double sp = 0.0, su = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        sp += pp[i];
        su += pu[i];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        sp += __shfl_xor(sp, o, kWave);
        su += __shfl_xor(su, o, kWave);
    }
    if (lane_id() == 0) {
        s_p[threadIdx.x >> 6] = sp;
        s_u[threadIdx.x >> 6] = su;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tp = 0.0, tu = 0.0;
        for (int w = 0; w < 16; ++w) {
            tp += s_p[w];
            tu += s_u[w];
        }
        norms[0] = tp;
        norms[1] = tu;
    }
}

// Dense second phase of the reference's momentum update (:122-131 Nesterov, :147-155 plain): it runs over
// the WHOLE parameter array every step, as the reference does.  Grid-stride stream; VEC = 4: float4 with the
// total & 3 tail elements done by the first workgroup, VEC = 1 (an array that is not 16-byte aligned, as every
// other optimizer here accepts): one element per thread, nvec == total.  Element for element the same arithmetic.
template <bool NESTEROV>
__device__ __forceinline__ void momentum_dense_step(float &p, float &v, float momentum) {
    if (NESTEROV) {
        const float t = momentum * v;
        v = t;
        p = p + t;
    } else {
        p = p + v;
        v = momentum * v;
    }
}

template <bool NESTEROV, int VEC>
__global__ __launch_bounds__(256) void momentum_dense_kernel(float *__restrict__ param,
                                                             float *__restrict__ veloc, float momentum,
                                                             uint64_t nvec, uint64_t total) {
    const uint64_t stride = static_cast<uint64_t>(gridDim.x) * 256u;
    for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; e < nvec; e += stride) {
        if (VEC == 4) {
            float4v p = ld4(param + e * 4), v = ld4(veloc + e * 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = p[k], vk = v[k];
                momentum_dense_step<NESTEROV>(pk, vk, momentum);
                p[k] = pk, v[k] = vk;
            }
            st4(param + e * 4, p);
            st4(veloc + e * 4, v);
        } else {
            momentum_dense_step<NESTEROV>(param[e], veloc[e], momentum);
        }
    }
    if (VEC == 4 && blockIdx.x == 0 && threadIdx.x < (total & 3u)) {   // tail elements
        const uint64_t e = (total & ~3ull) + threadIdx.x;
        momentum_dense_step<NESTEROV>(param[e], veloc[e], momentum);
    }
}

static bool vec_ok(int64_t width, const void *a, const void *b, const void *c, const void *d, const void *e) {
    auto al = [](const void *p) { return p == nullptr || reinterpret_cast<uintptr_t>(p) % 16 == 0; };
    return width % 4 == 0 && al(a) && al(b) && al(c) && al(d) && al(e);
}

template <int KIND>
static int row_launch(float *param, int64_t rows, const float *ids, float *grads, int64_t n, int64_t width,
                      float *s1, float *s2, const OptArgs &a, hipStream_t stream) {
    if (n == 0)
        return 0;
    unsigned blocks = static_cast<unsigned>((n + 3) / 4);
    if (blocks > 16384)
        blocks = 16384;
    if (vec_ok(width, param, grads, s1, s2, a.update))
        hipLaunchKernelGGL((sparse_row_kernel<KIND, 4>), dim3(blocks), dim3(256), 0, stream, param,
                           (uint64_t)rows, ids, grads, (int)n, (int)width, s1, s2, a);
    else
        hipLaunchKernelGGL((sparse_row_kernel<KIND, 1>), dim3(blocks), dim3(256), 0, stream, param,
                           (uint64_t)rows, ids, grads, (int)n, (int)width, s1, s2, a);
    HA_LAUNCH_CHECK();
    return 0;
}

static int check_args(const char *name, const DLArray *param, const DLArray *ids, const DLArray *grads,
                      const DLArray *s1, const DLArray *s2, bool need_s1, bool need_s2, int64_t *n,
                      int64_t *width) {
    HA_REQUIRE(param && ids && grads && (!need_s1 || s1) && (!need_s2 || s2), "%s: null array", name);
    HA_REQUIRE(param->data && ids->data && grads->data, "%s: null data pointer", name);
    HA_REQUIRE(param->ctx.device_type == kGPU && ids->ctx.device_type == kGPU && grads->ctx.device_type == kGPU,
               "%s: arrays must be on the GPU", name);
    if (need_s1)
        HA_REQUIRE(s1->data && s1->ctx.device_type == kGPU, "%s: state arrays must be on the GPU", name);
    if (need_s2)
        HA_REQUIRE(s2->data && s2->ctx.device_type == kGPU, "%s: state arrays must be on the GPU", name);
    HA_REQUIRE(param->ndim == 2, "%s: param must be 2-D", name);
    *n = dl_numel(ids);
    *width = param->shape[1];
    HA_REQUIRE(*n < (1ll << 31) && *width < (1ll << 30), "%s: sizes out of range", name);
    HA_REQUIRE(dl_numel(grads) == *n * *width, "%s: grad_values size mismatch", name);
    if (need_s1)
        HA_REQUIRE(dl_numel(s1) == dl_numel(param), "%s: state size mismatch", name);
    if (need_s2)
        HA_REQUIRE(dl_numel(s2) == dl_numel(param), "%s: state size mismatch", name);
    return 0;
}

}  // namespace ha

using namespace ha;

// src/ops/OptimizersSparse.cu:3-51 -- grad_values[i,:] += l2reg * param[indices[i],:]
extern "C" int AddL2RegularizationSparse(const DLArrayHandle param, const DLArrayHandle grad_indices,
                                         DLArrayHandle grad_values, float l2reg,
                                         DLStreamHandle stream_handle) {
    int64_t n, width;
    if (check_args("AddL2RegularizationSparse", param, grad_indices, grad_values, nullptr, nullptr, false, false,
                   &n, &width))
        return -1;
    OptArgs a{};
    a.weight_decay = l2reg;
    return row_launch<kL2>(static_cast<float *>(param->data), param->shape[0],
                           static_cast<const float *>(grad_indices->data),
                           static_cast<float *>(grad_values->data), n, width, nullptr, nullptr, a,
                           dl_stream(stream_handle));
}

// dense second phase of the momentum update over the whole table (momentum_dense_kernel)
static int momentum_dense(float *p, float *v, int64_t rows, int64_t width, float momentum, bool nesterov, hipStream_t stream) {
    const uint64_t total = static_cast<uint64_t>(rows) * static_cast<uint64_t>(width);
    if (total == 0)
        return 0;
    const bool vec = reinterpret_cast<uintptr_t>(p) % 16 == 0 && reinterpret_cast<uintptr_t>(v) % 16 == 0;
    const uint64_t nvec = vec ? total / 4 : total;
    uint64_t blocks = (nvec + 255) / 256;
    if (blocks > 65536)
        blocks = 65536;
    if (blocks == 0)
        blocks = 1;
    const dim3 grid(static_cast<unsigned>(blocks)), block(256);
    if (vec && nesterov)
        hipLaunchKernelGGL((momentum_dense_kernel<true, 4>), grid, block, 0, stream, p, v, momentum, nvec, total);
    else if (vec)
        hipLaunchKernelGGL((momentum_dense_kernel<false, 4>), grid, block, 0, stream, p, v, momentum, nvec, total);
    else if (nesterov)
        hipLaunchKernelGGL((momentum_dense_kernel<true, 1>), grid, block, 0, stream, p, v, momentum, nvec, total);
    else
        hipLaunchKernelGGL((momentum_dense_kernel<false, 1>), grid, block, 0, stream, p, v, momentum, nvec, total);
    HA_LAUNCH_CHECK();
    return 0;
}

// src/ops/OptimizersSparse.cu:101-231.  First phase (ids may repeat): velocity[id,:] += -lr * g per
// occurrence (Nesterov: param[id,:] too) -- here in occurrence order through the index plan instead of
// float atomics; acc - lr*g is bit for bit acc + (-lr*g).  Second phase: dense, over the whole table.
extern "C" int MomentumOptimizerSparseUpdate(DLArrayHandle param, const DLArrayHandle grad_indices,
                                             const DLArrayHandle grad_values, DLArrayHandle velocity,
                                             float lr, float momentum, bool nesterov,
                                             DLStreamHandle stream_handle) {
    int64_t n, width;
    if (check_args("MomentumOptimizerSparseUpdate", param, grad_indices, grad_values, velocity, nullptr, true,
                   false, &n, &width))
        return -1;
    hipStream_t stream = dl_stream(stream_handle);
    float *p = static_cast<float *>(param->data), *v = static_cast<float *>(velocity->data);
    const int64_t rows = param->shape[0];
    if (n > 0) {
        void *ws = nullptr;
        if (scratch_get(stream, ha_plan_bytes(n), &ws))
            return -1;
        if (ha_plan_sort_f32ids(static_cast<const float *>(grad_indices->data), n, ws, stream))
            return -1;
        const float *g = static_cast<const float *>(grad_values->data);
        if (ha_sgd_apply(v, rows, width, ws, n, g, lr, stream))
            return -1;
        if (nesterov && ha_sgd_apply(p, rows, width, ws, n, g, lr, stream))
            return -1;
    }
    return momentum_dense(p, v, rows, width, momentum, nesterov, stream);
}

// The one-call form on POOLED gradients (sum-pooled lookup, bagsum.hip): the first phase is ha_sgd_apply_bags -- occurrence i
// takes the row of its bag, nothing is expanded --, the second the same dense pass.  Bit for bit MomentumOptimizerSparseUpdate on
// bag_grads expanded to [n, width], in tolerance mode too (ha_sgd_apply_bags equals ha_sgd_apply there as well).
template <typename IdT>
static int momentum_sparse_update_bags(const char *what, float *param, int64_t rows, int64_t width, const IdT *ids, int64_t n,
                                       const float *bag_grads, int64_t bag, const int64_t *offsets, int64_t nbags,
                                       float *velocity, float lr, float momentum, int nesterov, ha_stream_t stream) {
    HA_REQUIRE(rows >= 0 && width >= 1 && width < (1ll << 30) && n >= 0 && n < (1ll << 31) && nbags >= 0 && bag >= 0 &&
                   nbags < (1ll << 31),
               "%s: bad sizes rows=%ld width=%ld n=%ld bag=%ld nbags=%ld", what, (long)rows, (long)width, (long)n, (long)bag,
               (long)nbags);
    HA_REQUIRE((bag >= 1) != (offsets != nullptr), "%s: give exactly one of bag >= 1 and offsets (bag=%ld)", what, (long)bag);
    HA_REQUIRE(offsets != nullptr || (n % bag == 0 && n / bag == nbags), "%s: n=%ld is not nbags=%ld bags of bag=%ld ids", what,
               (long)n, (long)nbags, (long)bag);
    HA_REQUIRE(param && velocity && (n == 0 || (ids && bag_grads && nbags >= 1)), "%s: null pointer or no bags", what);
    hipStream_t s = as_stream(stream);
    if (n > 0) {
        const size_t plan_bytes = align_up(ha_plan_bytes(n), 256);
        void *ws = nullptr;
        if (scratch_get(s, plan_bytes + (offsets ? static_cast<size_t>(n) * 4 : 0), &ws))
            return -1;
        int32_t *bag_of = nullptr;
        if (offsets) {
            bag_of = reinterpret_cast<int32_t *>(static_cast<char *>(ws) + plan_bytes);
            if (ha_bag_of(offsets, nbags, n, bag_of, stream))
                return -1;
        }
        if (sizeof(IdT) == 4 ? ha_plan_sort_f32ids(reinterpret_cast<const float *>(ids), n, ws, stream)
                             : ha_plan_sort_u64ids(reinterpret_cast<const uint64_t *>(ids), n, ws, stream))
            return -1;
        if (ha_sgd_apply_bags(velocity, rows, width, ws, n, bag_grads, offsets ? 0 : bag, bag_of, lr, stream))
            return -1;
        if (nesterov && ha_sgd_apply_bags(param, rows, width, ws, n, bag_grads, offsets ? 0 : bag, bag_of, lr, stream))
            return -1;
    }
    return momentum_dense(param, velocity, rows, width, momentum, nesterov != 0, s);
}

extern "C" int ha_momentum_sparse_update_bags_f32ids(float *param, int64_t rows, int64_t width, const float *ids, int64_t n,
                                                     const float *bag_grads, int64_t bag, const int64_t *offsets,
                                                     int64_t nbags, float *velocity, float lr, float momentum, int nesterov,
                                                     ha_stream_t stream) {
    return momentum_sparse_update_bags<float>("ha_momentum_sparse_update_bags_f32ids", param, rows, width, ids, n, bag_grads,
                                              bag, offsets, nbags, velocity, lr, momentum, nesterov, stream);
}

extern "C" int ha_momentum_sparse_update_bags_u64ids(float *param, int64_t rows, int64_t width, const uint64_t *ids, int64_t n,
                                                     const float *bag_grads, int64_t bag, const int64_t *offsets,
                                                     int64_t nbags, float *velocity, float lr, float momentum, int nesterov,
                                                     ha_stream_t stream) {
    return momentum_sparse_update_bags<uint64_t>("ha_momentum_sparse_update_bags_u64ids", param, rows, width, ids, n, bag_grads,
                                                 bag, offsets, nbags, velocity, lr, momentum, nesterov, stream);
}

extern "C" int AdaGradOptimizerSparseUpdate(DLArrayHandle param, const DLArrayHandle grad_indices,
                                            const DLArrayHandle grad_values, DLArrayHandle acc, float lr,
                                            float eps, DLStreamHandle stream_handle) {
    int64_t n, width;
    if (check_args("AdaGradOptimizerSparseUpdate", param, grad_indices, grad_values, acc, nullptr, true, false,
                   &n, &width))
        return -1;
    OptArgs a{};
    a.lr = lr;
    a.eps = eps;
    return row_launch<kAdaGrad>(static_cast<float *>(param->data), param->shape[0],
                                static_cast<const float *>(grad_indices->data),
                                static_cast<float *>(grad_values->data), n, width,
                                static_cast<float *>(acc->data), nullptr, a, dl_stream(stream_handle));
}

static OptArgs adam_args(float lr, float beta1, float beta2, float beta1t, float beta2t, float eps, float wd) {
    OptArgs a{};
    a.lr = lr, a.eps = eps, a.beta1 = beta1, a.beta2 = beta2, a.beta1t = beta1t, a.beta2t = beta2t;
    a.weight_decay = wd;
    return a;
}

extern "C" int AdamOptimizerSparseUpdate(DLArrayHandle param, const DLArrayHandle grad_indices,
                                         const DLArrayHandle grad_values, DLArrayHandle expavg,
                                         DLArrayHandle expavgsq, float lr, float beta1, float beta2,
                                         float beta1t, float beta2t, float eps, DLStreamHandle stream_handle) {
    int64_t n, width;
    if (check_args("AdamOptimizerSparseUpdate", param, grad_indices, grad_values, expavg, expavgsq, true, true, &n,
                   &width))
        return -1;
    return row_launch<kAdam>(static_cast<float *>(param->data), param->shape[0],
                             static_cast<const float *>(grad_indices->data),
                             static_cast<float *>(grad_values->data), n, width,
                             static_cast<float *>(expavg->data), static_cast<float *>(expavgsq->data),
                             adam_args(lr, beta1, beta2, beta1t, beta2t, eps, 0.f), dl_stream(stream_handle));
}

extern "C" int AdamWOptimizerSparseUpdate(DLArrayHandle param, const DLArrayHandle grad_indices,
                                          const DLArrayHandle grad_values, DLArrayHandle expavg,
                                          DLArrayHandle expavgsq, float lr, float beta1, float beta2,
                                          float beta1t, float beta2t, float eps, float weight_decay,
                                          DLStreamHandle stream_handle) {
    int64_t n, width;
    if (check_args("AdamWOptimizerSparseUpdate", param, grad_indices, grad_values, expavg, expavgsq, true, true,
                   &n, &width))
        return -1;
    return row_launch<kAdamW>(static_cast<float *>(param->data), param->shape[0],
                              static_cast<const float *>(grad_indices->data),
                              static_cast<float *>(grad_values->data), n, width,
                              static_cast<float *>(expavg->data), static_cast<float *>(expavgsq->data),
                              adam_args(lr, beta1, beta2, beta1t, beta2t, eps, weight_decay),
                              dl_stream(stream_handle));
}

// src/ops/OptimizersSparse.cu:524-722 (deduplicated slices): norm2 of the indexed parameter rows, Adam
// moments + update direction, norm2 of the direction, then
//   param[id,:] -= lr * (norm2_param / norm2_update) * (update + weight_decay * param[id,:]).
// Three launches: direction + per-row partial norms, the two sums, the step.
extern "C" int LambOptimizerSparseUpdate(DLArrayHandle param, const DLArrayHandle grad_indices,
                                         const DLArrayHandle grad_values, DLArrayHandle expavg,
                                         DLArrayHandle expavgsq, float lr, float beta1, float beta2,
                                         float beta1t, float beta2t, float eps, float weight_decay,
                                         DLStreamHandle stream_handle) {
    int64_t n, width;
    if (check_args("LambOptimizerSparseUpdate", param, grad_indices, grad_values, expavg, expavgsq, true, true, &n,
                   &width))
        return -1;
    if (n == 0)
        return 0;
    hipStream_t stream = dl_stream(stream_handle);
    const size_t upd_bytes = align_up(static_cast<size_t>(n) * width * 4, 256);
    const size_t part_bytes = align_up(static_cast<size_t>(n) * 8, 256);
    void *ws = nullptr;
    if (scratch_get(stream, upd_bytes + 2 * part_bytes + 256, &ws))
        return -1;
    char *b = static_cast<char *>(ws);
    OptArgs a = adam_args(lr, beta1, beta2, beta1t, beta2t, eps, weight_decay);
    a.update = reinterpret_cast<float *>(b);
    a.part_param = reinterpret_cast<double *>(b + upd_bytes);
    a.part_update = reinterpret_cast<double *>(b + upd_bytes + part_bytes);
    double *norms = reinterpret_cast<double *>(b + upd_bytes + 2 * part_bytes);
    a.norms = norms;
    float *p = static_cast<float *>(param->data);
    const float *ids = static_cast<const float *>(grad_indices->data);
    float *g = static_cast<float *>(grad_values->data);
    if (row_launch<kLambUpdate>(p, param->shape[0], ids, g, n, width, static_cast<float *>(expavg->data),
                                static_cast<float *>(expavgsq->data), a, stream))
        return -1;
    hipLaunchKernelGGL(lamb_norms_kernel, dim3(1), dim3(1024), 0, stream, a.part_param, a.part_update, (int)n,
                       norms);
    HA_LAUNCH_CHECK();
    return row_launch<kLambStep>(p, param->shape[0], ids, g, n, width, nullptr, nullptr, a, stream);
}
