// Per-token confidence and top-K alternatives of one joiner round (DESIGN.md section 12).  Included by kernels_misc.hip;
// the decision kernel (decide_body<true>, launched as decide_conf_kernel once a session of the engine has opted in) calls
// confidence_row for rows whose session opted in, AFTER the round's StepRecord and decision are written: nothing here feeds
// back into the search.
//
// For the row's logits v[0..V) -- the same expression, hence the same bits, the arg-max compared:
//   M = max v (blank included), S = sum expf(v - M), lse = M + logf(S);
//   alternatives = the non-blank ids by (v descending, id ascending), the first K.
// Order of the sum: lane t of the 256 adds its terms n = t, t + 256, ... in that order, the 64 lanes of a wave are combined by
// an xor butterfly (6 additions), the four wave sums are added as ((w0 + w1) + w2) + w3: a fixed function of (V, row), at most
// ceil(V / 256) + 8 additions on any term's path (V <= 6144 keeps that within the contract's 32).
// All 256 threads of the workgroup call it (it synchronises); the branch around the call is uniform.

constexpr int kConfRegs = 4;                       // logits each lane keeps in registers (V <= 1024); the rest is re-evaluated per pass

// `bonus`: the row's phrase-boosting table in LDS (kernels_bias.inc; DESIGN.md section 13) or null -- the search of a biased session
// compares v' = v + bonus, and so do the confidences
__device__ __forceinline__ float conf_logit(const DecideArgs &a, int m, int n, const float *bonus)
{
    const float v = tree_sum(a.ws, a.parts, a.m_stride, a.N, m, n) + a.bias[n];
    return bonus ? bias_apply(v, bonus[n]) : v;
}

// a strict set's forbidden token: the search did not compare it, so it is in no pass below -- not in the maximum, not a term of the
// sum (skipped, not added as zero), never an alternative.  The blank is always permitted.
__device__ __forceinline__ bool conf_skip(const DecideArgs &a, int n, const float *bonus)
{
    return bonus && n != a.blank && bias_forbidden(bonus[n]);
}

// (value, id) arg-max over the workgroup with the search's order: higher value first, lower id on ties; id < 0 = nothing.
// One barrier per call: the LDS cells alternate with `phase`, so a call never overwrites cells another wave may still read.
__device__ __forceinline__ void conf_block_best(float &v, int &i, float (*s_v)[4], int (*s_i)[4], int phase)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
    }
    if ((threadIdx.x & 63) == 0) { s_v[phase][threadIdx.x >> 6] = v; s_i[phase][threadIdx.x >> 6] = i; }
    __syncthreads();
    v = s_v[phase][0]; i = s_i[phase][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const float ov = s_v[phase][w]; const int oi = s_i[phase][w];
        if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
    }
}

__device__ __forceinline__ void confidence_row(const DecideArgs &a, int m, int K, ConfRecord *out, const float *bonus = nullptr)
{
    __shared__ float s_v[2][4], s_f[2][4];
    __shared__ int s_i[2][4];
    const int tid = threadIdx.x;
    const int V = a.n_valid;
    float c[kConfRegs];
    unsigned skip = 0;                                           // bit j: c[j] belongs to a forbidden token (conf_skip)

    // pass 1: the row maximum (blank included) and the arg-max the StepRecord holds (same comparison, same initial value)
    float mx = -INFINITY;
    float best = -9999999999.0f;
    int best_i = -1;
#pragma unroll
    for (int j = 0; j < kConfRegs; ++j) {
        const int n = tid + 256 * j;
        c[j] = 0.0f;
        if (n < V && conf_skip(a, n, bonus)) skip |= 1u << j;
        else if (n < V) {
            const float v = c[j] = conf_logit(a, m, n, bonus);
            mx = fmaxf(mx, v);
            if (n != a.blank && v > best) { best = v; best_i = n; }
        }
    }
    for (int n = tid + 256 * kConfRegs; n < V; n += 256) {
        if (conf_skip(a, n, bonus)) continue;
        const float v = conf_logit(a, m, n, bonus);
        mx = fmaxf(mx, v);
        if (n != a.blank && v > best) { best = v; best_i = n; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if ((tid & 63) == 0) s_f[0][tid >> 6] = mx;
    conf_block_best(best, best_i, s_v, s_i, 0);                  // (its barrier also publishes s_f[0])
    mx = fmaxf(fmaxf(s_f[0][0], s_f[0][1]), fmaxf(s_f[0][2], s_f[0][3]));

    if (best_i < 0) {                                            // no logit beat the initial value (NaNs): StepRecord.idx == -1
        if (tid == 0) {
            out->lse = __builtin_nanf(""); out->blank_val = conf_logit(a, m, a.blank, bonus); out->n_alt = 0; out->reserved = 0;
            for (int k = 0; k < kConfMaxAlt; ++k) { out->alt_id[k] = -1; out->alt_logit[k] = 0.0f; }
        }
        return;
    }

    // pass 2: sum of exponentials in the fixed order stated above
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < kConfRegs; ++j)
        if (tid + 256 * j < V && !(skip >> j & 1)) sum += expf(c[j] - mx);
    for (int n = tid + 256 * kConfRegs; n < V; n += 256)
        if (!conf_skip(a, n, bonus)) sum += expf(conf_logit(a, m, n, bonus) - mx);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if ((tid & 63) == 0) s_f[1][tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        const float S = ((s_f[1][0] + s_f[1][1]) + s_f[1][2]) + s_f[1][3];
        out->lse = mx + logf(S);
        out->blank_val = conf_logit(a, m, a.blank, bonus);
        out->reserved = 0;
        out->alt_id[0] = best_i; out->alt_logit[0] = best;
    }

    // alternatives 1 .. K-1: the best candidate that comes after the previous pick in (value descending, id ascending) order
    int n_alt = 1;
    float pv = best;
    int pi = best_i;
    for (int k = 1; k < K; ++k) {
        float bv = 0.0f;
        int bi = -1;
        auto offer = [&](float v, int n) {
            const bool after = v < pv || (v == pv && n > pi);
            if (n != a.blank && after && (bi < 0 || v > bv)) { bv = v; bi = n; }      // (ids ascend within a lane: '>' keeps the lower id)
        };
#pragma unroll
        for (int j = 0; j < kConfRegs; ++j)
            if (tid + 256 * j < V && !(skip >> j & 1)) offer(c[j], tid + 256 * j);
        for (int n = tid + 256 * kConfRegs; n < V; n += 256)
            if (!conf_skip(a, n, bonus)) offer(conf_logit(a, m, n, bonus), n);
        conf_block_best(bv, bi, s_v, s_i, k & 1);
        if (bi < 0) break;                                       // fewer than K candidates (uniform: every thread holds the same result)
        if (tid == 0) { out->alt_id[k] = bi; out->alt_logit[k] = bv; }
        pv = bv; pi = bi;
        n_alt = k + 1;
    }
    if (tid == 0) {
        out->n_alt = n_alt;
        for (int k = n_alt; k < kConfMaxAlt; ++k) { out->alt_id[k] = -1; out->alt_logit[k] = 0.0f; }
    }
}
