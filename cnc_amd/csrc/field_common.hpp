// field_common.hpp — device helpers shared by the radiance field's glue kernels (field_glue.hip) and the fused
// positions -> density / rgb kernel (field_fused.hip).
#pragma once

#include <hip/hip_fp16.h>

#include "common.hpp"

namespace cnc {

// four of the 16 terms of sh4 (same expressions): q = 0..3 -> terms 4q .. 4q+3
__device__ __forceinline__ float4 sh4_quad(uint32_t q, float x, float y, float z)
{
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    switch (q) {
    case 0: return make_float4(0.28209479177387814f, -0.48860251190291987f * y, 0.48860251190291987f * z,
                               -0.48860251190291987f * x);
    case 1: return make_float4(1.0925484305920792f * xy, -1.0925484305920792f * yz,
                               0.94617469575755997f * zz - 0.31539156525251999f, -1.0925484305920792f * xz);
    case 2: return make_float4(0.54627421529603959f * xx - 0.54627421529603959f * yy,
                               0.59004358992664352f * y * (-3.0f * xx + yy), 2.8906114426405538f * xy * z,
                               0.45704579946446572f * y * (1.0f - 5.0f * zz));
    default: return make_float4(0.3731763325901154f * z * (5.0f * zz - 3.0f), 0.45704579946446572f * x * (1.0f - 5.0f * zz),
                                1.4453057213202769f * z * (xx - yy), 0.59004358992664352f * x * (-xx + 3.0f * yy));
    }
}

// World position -> the position the encoders see, + the selector: the ONE definition behind cnc_field_prepare,
// cnc_field_prepare_contracted and every form of cnc_field_fused_forward (the arithmetic is spelled out in
// include/cnc_hip.h, CNC_FIELD_CONTRACT; tests/contract_twin.py restates it in NumPy).  `pw`: the sample's three world
// coordinates in memory; `aext` = max - min.
// contract = false: x = (p - min) / (max - min) (ngp.py:516-521).  contract = true: contract_to_unisphere (ngp.py:337-361,
// ord = 2) on top of it.  Nothing fuses (-ffp-contract=off); `/` and sqrtf are correctly rounded under the build's flags
// (hipcc's default; __fsqrt_rn is NOT: it is the native square root, 1 ulp).
__device__ __forceinline__ bool field_unit_position(const float* __restrict__ pw, const float (&amin)[3], const float (&aext)[3],
                                                    bool contract, float (&x)[3])
{
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        x[a] = (pw[a] - amin[a]) / aext[a];
        if (!contract) in = in && x[a] > 0.0f && x[a] < 1.0f;
    }
    if (contract) {
        float c[3];
#pragma unroll
        for (int a = 0; a < 3; a++) c[a] = x[a] * 2.0f - 1.0f;
        const float mag = sqrtf((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
        if (mag > 1.0f) {
            const float k = 2.0f - 1.0f / mag;
#pragma unroll
            for (int a = 0; a < 3; a++) c[a] = k * (c[a] / mag);
        }
#pragma unroll
        for (int a = 0; a < 3; a++) {
            x[a] = c[a] / 4.0f + 0.5f;
            in = in && x[a] > 0.0f && x[a] < 1.0f;
        }
    }
    return in;
}

// tiny-cuda-nn stores its encodings as half (CNC_FIELD_SH_FP16, include/cnc_hip.h)
__device__ __forceinline__ float round_through_half(float v) { return __half2float(__float2half_rn(v)); }

}  // namespace cnc
