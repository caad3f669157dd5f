// The arithmetic behind the reductions, stated once (included from device_utils.h).  The build uses -ffp-contract=off, so the written
// order of operations decides the bits: every schedule of a GEMM (kernels_gemm*.hip, kernels_recur.hip) and the row kernels that
// finish the split-K forms (kernels_misc.hip) call these functions, and a session computes the same bits whichever of them its batch
// size selects.  They are functions of registers: where a kernel fetches the operands and how it stores the results (and where it
// waits for memory) stays with the kernel.
#pragma once

namespace aprilx {

using h4 = __attribute__((ext_vector_type(4))) _Float16;
__device__ __forceinline__ h4 to_h4(const f32x4 &v) { return h4{(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w}; }

// DoubleSwish y * sigma(y - 1) (EPI_BIAS_DSWISH, the convolutional front end)
__device__ __forceinline__ float dswish(float y) { return y * fast_sigmoid(y - 1.0f); }
__device__ __forceinline__ f32x4 dswish4(const f32x4 &y)
{
    f32x4 o;
    o.x = y.x * fast_sigmoid(y.x - 1.0f); o.y = y.y * fast_sigmoid(y.y - 1.0f);
    o.z = y.z * fast_sigmoid(y.z - 1.0f); o.w = y.w * fast_sigmoid(y.w - 1.0f);
    return o;
}

// LSTM cell of one hidden unit (EPI_LSTM): gt = pre-activations of the gates i, f, g, o
struct LstmCell { float c_new, u; };
__device__ __forceinline__ LstmCell lstm_cell(const f32x4 &gt, float c_prev)
{
    const float c_new = fast_sigmoid(gt.y) * c_prev + fast_sigmoid(gt.x) * fast_tanh(gt.z);
    return LstmCell{c_new, fast_sigmoid(gt.w) * fast_tanh(c_new)};
}

// Gate pre-activations of the fp32 chunk form (kernels.h): ((xin + p2) + p3) + bias, where xin is the input half of the slab, either
// the chunks (p0 + p1) * scale(y) of this launch or the quad EPI_XPART left for all time steps (layer-major, p_add).  (The fp16
// one-chain forms hold one accumulator and only add the bias.)
__device__ __forceinline__ f32x4 gate_xin(const f32x4 &p0, const f32x4 &p1, float scale) { return (p0 + p1) * scale; }
__device__ __forceinline__ f32x4 gate_combine(const f32x4 &xin, const f32x4 &p2, const f32x4 &p3, const f32x4 &bias) { return ((xin + p2) + p3) + bias; }

// LSTM projection (EPI_HR / ROW_HR): the sum is the new h state; the layer goes on with x + h', x = resid * scale(resid)
struct HrTail { f32x4 state, out; };
__device__ __forceinline__ HrTail hr_tail(const f32x4 &v, const f32x4 &resid, float rs) { return HrTail{v, resid * rs + v}; }

// EPI_RESID_SSQ / ROW_RESID_SSQ: y = resid + (v + bias), the residual optional
__device__ __forceinline__ f32x4 resid_tail(const f32x4 &v, const f32x4 &bias, const f32x4 &resid, bool has_resid)
{
    f32x4 y = v + bias;
    if (has_resid) y = resid + y;
    return y;
}
// ... and the sum of squares of y's granule (granule_ssq: every lane of the wave calls this, rows that are not stored with y = 0);
// true for the lane that stores it: the first of the granule's eight quads (q = the quad's number within its row)
__device__ __forceinline__ bool granule_ssq_store(const f32x4 &y, bool ok, int q, float &ss)
{
    ss = granule_ssq(y);
    return ok && (q & 7) == 0;
}

// EPI_SLOT_STORE / ROW_SLOT_STORE: bias on the sum, or on the sum of a GEMM over y times the row's scale
__device__ __forceinline__ f32x4 slot_value(const f32x4 &v, const f32x4 &bias) { return v + bias; }
__device__ __forceinline__ f32x4 slot_value(const f32x4 &v, float scale, const f32x4 &bias) { return v * scale + bias; }

// The BasicNorm scales of a tile's BM rows through LDS.  The rows' sum-of-squares partials are parked as part[row * (G + 1) + j]
// (G = rsc.groups; the padding makes the column walks conflict-free), either from the registers that have held them since the first
// instruction of the kernel (staged: thread t holds partials sj0 .. sj0 + ppt - 1 of row srow in stg) or, where a row has more partials
// than the stage registers take, fetched now through `load`.  Behind a barrier of the caller's, one thread per row adds the row's
// partials in column order -- the order of row_scale() -- with rows_scale_sum.
template <int BM, int NTH, int NSTG, class Load>
__device__ __forceinline__ void rows_scale_park(float *part, const RowScale &rsc, bool staged, const float (&stg)[NSTG], int ppt, int srow, int sj0, int m0, int M, Load load)
{
    const int G = rsc.groups;
    if (staged) {
#pragma unroll
        for (int k = 0; k < NSTG; ++k) if (k < ppt && sj0 + k < G) part[srow * (G + 1) + sj0 + k] = stg[k];
    } else {
        for (int i = threadIdx.x; i < BM * G; i += NTH) {
            int r = m0 + i / G;
            if (r >= M) r = M - 1;
            part[(i / G) * (G + 1) + i % G] = load(rsc.ssq + (size_t)r * G + i % G);
        }
    }
}
__device__ __forceinline__ float rows_scale_sum(const float *row_part, const RowScale &rsc)
{
    float t = 0.0f;
    for (int j = 0; j < rsc.groups; ++j) t += row_part[j];
    return __builtin_amdgcn_rsqf(t * rsc.inv_n + rsc.eps);
}

}  // namespace aprilx
