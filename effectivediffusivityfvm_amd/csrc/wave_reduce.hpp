// wave_reduce.hpp -- wavefront-level (wave64) lane shifts and the fixed-order DPP sum tree shared by the residual
// (kernels_residual.hpp), conjugate-gradient (kernels_cg.hpp) and gradient-pass (kernels_facepass.hpp) reductions, and the
// final sum of an image's partial sums that the residual and the gradient passes end with.
#pragma once
#include <hip/hip_runtime.h>

namespace deff {

template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ double dpp_f64(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, BANK_MASK, true);     // lanes without a source read 0
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, BANK_MASK, true);
    return __hiloint2double(hi, lo);
}
// lane i <- lane i - 1 (wave_shr:1) / lane i + 1 (wave_shl:1); the lane without a source (0 / 63) keeps `edge`
template <int CTRL>
__device__ __forceinline__ double dpp_f64_keep(double v, double edge)
{
    int lo = __builtin_amdgcn_update_dpp(__double2loint(edge), __double2loint(v), CTRL, 0xf, 0xf, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(edge), __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32_keep(unsigned v, unsigned edge)
{
    return (unsigned)__builtin_amdgcn_update_dpp((int)edge, (int)v, CTRL, 0xf, 0xf, false);
}

// Sum of the 64 lanes' values; valid in lane 63.  Fixed order: within a row of 16 lanes prefix sums by row_shr 1, 2, 3, then
// 4 and 8; rows 1 and 3 add lane 15 of the row below (row_bcast:15), rows 2 and 3 add lane 31 (row_bcast:31).
__device__ __forceinline__ double wave_sum_to_lane63(double v)
{
    double t = v + dpp_f64<0x111, 0xf, 0xf>(v);                  // row_shr:1
    t = t + dpp_f64<0x112, 0xf, 0xf>(v);                         // row_shr:2
    t = t + dpp_f64<0x113, 0xf, 0xf>(v);                         // row_shr:3   -> t[i] = v[i-3..i]
    t = t + dpp_f64<0x114, 0xf, 0xe>(t);                         // row_shr:4, banks 1-3
    t = t + dpp_f64<0x118, 0xf, 0xc>(t);                         // row_shr:8, banks 2-3 -> lane 15 of a row = the row's sum
    t = t + dpp_f64<0x142, 0xa, 0xf>(t);                         // row_bcast:15 into rows 1 and 3
    t = t + dpp_f64<0x143, 0xc, 0xf>(t);                         // row_bcast:31 into rows 2 and 3
    return t;
}

// The body of a __global__ __launch_bounds__(1024) kernel, one workgroup of 16 waves per image: thread t adds the partial sums
// t, t + 1024, ... of its image in that order, the wave tree combines the 64 thread sums of a wave, thread 0 adds the 16 wave
// sums in wave order.  out[img] = sum.  (k_residual_final, k_pass_final: one order, one text.)
__device__ __forceinline__ void partials_sum_body(const double *__restrict__ partial, size_t per_img, double *__restrict__ out)
{
    __shared__ double ws[16];
    const double *p = partial + (size_t)blockIdx.x * per_img;
    double acc = 0.0;
    size_t i = threadIdx.x;
    for (; i + 3 * 1024 < per_img; i += 4 * 1024) {               // four loads in flight, added in index order
        const double a = p[i], b = p[i + 1024], c = p[i + 2048], d = p[i + 3072];
        acc += a; acc += b; acc += c; acc += d;
    }
    for (; i < per_img; i += 1024) acc += p[i];
    const double s = wave_sum_to_lane63(acc);
    if ((threadIdx.x & 63) == 63) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = ws[0];
#pragma unroll
        for (int w = 1; w < 16; ++w) t += ws[w];
        out[blockIdx.x] = t;
    }
}

}  // namespace deff
