// Phrase boosting inside the joiner decision (DESIGN.md section 13).  Included by kernels_misc.hip; used by the BIAS forms of
// decide_body (decide_bias_kernel / decide_conf_bias_kernel, launched once a session of the engine has opted in).
//
// For a row whose slot has a bias set, the slot's trie state s selects the effective edges [state_off[s], state_off[s + 1]):
// token -> (bonus, next state).  The workgroup spreads them into a DENSE table in dynamic LDS -- bonus[V] (fp32) and next[V]
// (16 bit; a set has at most 65535 states) --: every cell is first set to "no edge", then the edges are scattered, so that the
// arg-max loop, the passes of confidence_row and the state update read bonus(s, n) / next(s, n) with one LDS load.  The other
// obvious form, the edge list staged in LDS and a binary search per logit, costs log2(edges) DEPENDENT LDS reads for each of the
// ceil(V / 256) logits of a lane and again in every pass of confidence_row; the dense form costs V / 256 stores and
// edges / 256 load-store pairs per lane once, and 6 bytes of LDS per token (V <= 8192, checked on the host).
// A token without an edge gets NO addition (not "+ 0"), so the row's other logits keep their bits.
// Vector stores only, no atomics; thread 0 writes the new state beside the GreedyState.
//
// Strict sets (BiasDesc::flags & 1: a closed phrase list): the edges of a state are the tokens PERMITTED there, and the table is
// filled with a third cell value, "forbidden", in place of "no edge" -- the scatter is the same.  A forbidden non-blank token takes no
// part in the arg-max (bias_scan) nor in any pass of confidence_row, exactly as the blank takes none in the arg-max; the blank's own
// cell is never scattered to and is not consulted (the blank is always permitted, never biased).  A row with nothing permitted above
// the initial value leaves best_i == -1, which decide_body's unchanged lines resolve (to blank, unless the blank logit is a NaN).
// bias_row_end needs no case of its own: next[] of a forbidden token is the root's 0.

constexpr unsigned kBiasNoEdge = 0x7fc0b1a5u;      // a NaN pattern: boosts are finite, so no edge's bonus has these bits
constexpr unsigned kBiasForbidden = 0x7fc0f0bdu;   // another one: the fill value of a strict set's table

__device__ __forceinline__ bool bias_forbidden(float cell) { return __float_as_uint(cell) == kBiasForbidden; }

// (not called for a forbidden cell, except for the blank's, which never holds a bonus)
__device__ __forceinline__ float bias_apply(float v, float cell)
{
    return __float_as_uint(cell) == kBiasNoEdge || bias_forbidden(cell) ? v : v + cell;
}

struct BiasRow {
    const float *bonus = nullptr;                  // LDS [V], null: the row's slot has no set (uniform per workgroup)
    const unsigned short *next = nullptr;          // LDS [V]
    int state = 0;
};

__host__ __device__ inline size_t bias_lds_bytes(int V) { return (size_t)V * 4 + (((size_t)V * 2 + 15) & ~(size_t)15); }

// All 256 threads of the workgroup call it (it synchronises when the slot has a set).
__device__ __forceinline__ void bias_row_begin(const DecideArgs &a, int m, unsigned char *lds, BiasRow &br)
{
    const int slot = a.slot_idx[m];
    const int set = a.bias_set[slot];
    if (set < 0) return;
    const BiasDesc d = a.bias_desc[set];
    int s = a.bias_state[slot];
    if ((unsigned)s >= (unsigned)d.n_states) s = 0;
    const int e0 = d.state_off[s], e1 = d.state_off[s + 1];
    const int V = a.n_valid;
    float *bonus = reinterpret_cast<float *>(lds);
    unsigned short *next = reinterpret_cast<unsigned short *>(lds + (size_t)V * 4);
    const float fill = __uint_as_float((d.flags & 1) ? kBiasForbidden : kBiasNoEdge);
    for (int n = threadIdx.x; n < V; n += 256) { bonus[n] = fill; next[n] = 0; }
    __syncthreads();
    for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {
        const int t = d.edge_tok[e];
        if ((unsigned)t < (unsigned)V) { bonus[t] = d.edge_bonus[e]; next[t] = (unsigned short)d.edge_next[e]; }
    }
    __syncthreads();
    br.bonus = bonus; br.next = next; br.state = s;
}

// decide_body's arg-max loop on v' = v + bonus(s, n): the same statements, the bonus added between the logit dump (which keeps
// the network's output) and the comparisons.  It is a COPY of that loop (whose lines stay as they are for the mutation yardstick,
// tests/mutate_device_decide.py, which edits the original in its first list and this copy in its list of the opt-in lines): any change
// to one has to be made in the other.
__device__ __forceinline__ void bias_scan(const DecideArgs &a, int m, const BiasRow &br, float &best, int &best_i, float &blank_v)
{
    for (int n = threadIdx.x; n < a.n_valid; n += 256) {
        const float raw = tree_sum(a.ws, a.parts, a.m_stride, a.N, m, n) + a.bias[n];
        if (a.logits_dump) a.logits_dump[(size_t)m * a.n_valid + n] = raw;
        const float cell = br.bonus[n];
        const float v = bias_apply(raw, cell);
        if (n == a.blank) blank_v = v;
        else if (bias_forbidden(cell)) continue;                 // strict set: not permitted from this state
        else if (v > best) { best = v; best_i = n; }
    }
}

// thread 0, after the decision: a non-blank decision follows the token's effective edge (else the root); the silence branch (>= 2200 ms, or
// the session's own endpoint silence) returns to the root whether or not the context was cleared
__device__ __forceinline__ void bias_row_end(const DecideArgs &a, const BiasRow &br, int slot, bool is_blank, int tok, bool silence)
{
    int s = br.state;
    if (!is_blank) s = br.next[tok];
    else if (silence) s = 0;
    a.bias_state[slot] = s;
}
