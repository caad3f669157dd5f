// Text-corpus language model inside the joiner decision (DESIGN.md section 20).  Included by kernels_misc.hip; used by the LM forms of
// decide_body (decide_lm_kernel and its CONF / OPT siblings, launched once a session of the engine has a model).  The LM forms are
// instantiated on top of BIAS = true and reuse its dense LDS table (kernels_bias.inc): for a row whose slot has a model, after
// bias_row_begin has filled and scattered -- or, on a row without a bias set, after a fill alone -- every lane walks its ceil(V / 256)
// tokens through the model's back-off automaton from the slot's node and combines
//     term = w * score(s, n) + b                      (the product rounded, then the sum: the file is compiled without contraction)
// into cell[n]: `term` where the cell held "no edge", `bonus + term` (one fp32 addition) where it held a bonus; a forbidden cell and the
// blank's cell stay what they are.  One barrier, then bias_scan, confidence_row, the strict mask and bias_row_end run as they are: they
// read v' = v + cell with one LDS load per token.
// The walk (lm.h states the same lines for the host): per byte, the arc of the node for that byte (binary search in the node's sorted
// arcs) adds its logp and moves on; without one the node's back-off weight is added and the walk repeats from back[s]; at the root an
// unseen byte costs unk_logp.  All additions are fp32, in the order written.  This is the plain CSR form: the device copy carries no
// acceleration table beside it.
// A row whose slot has no model pays one uniform 16-byte load (its LmSlot) and then runs the BIAS lines.
// Plain C++, vector loads and stores only, no atomics; thread 0 re-walks the decided token and writes the new node beside the bias state.

struct LmRow {
    int model = -1;                                // uniform per workgroup; < 0: the row's slot has no model
    int state = 0;
    bool bias = false;                             // the slot has a bias set as well (bias_row_end runs)
};

struct LmNoRow {};

// arc of node s for byte c, or -1
__device__ __forceinline__ int lm_find(const LmDesc &d, int s, unsigned c)
{
    int lo = d.node_off[s];
    const int end = d.node_off[s + 1];
    int hi = end;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((unsigned)d.arc_byte[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo < end && (unsigned)d.arc_byte[lo] == c ? lo : -1;
}

// score(s, tok): returns acc, moves s.  back[] of a node is a node of a shorter context, so the inner loop ends at the root at the latest.
__device__ __forceinline__ float lm_walk(const LmDesc &d, int &s, int tok)
{
    float acc = 0.0f;
    const int b1 = d.tok_off[tok + 1];
    for (int i = d.tok_off[tok]; i < b1; ++i) {
        const unsigned c = d.tok_bytes[i];
        for (;;) {
            const int e = lm_find(d, s, c);
            if (e >= 0) { acc = acc + d.arc_logp[e]; s = d.arc_next[e]; break; }
            if (s == 0) { acc = acc + d.unk_logp; break; }
            acc = acc + d.bow[s]; s = d.back[s];
        }
    }
    return acc;
}

// All 256 threads of the workgroup call it, after bias_row_begin (it synchronises when the slot has a model).
__device__ __forceinline__ void lm_row_begin(const DecideArgs &a, int m, unsigned char *lds, BiasRow &br, LmRow &lr)
{
    const int slot = a.slot_idx[m];
    const LmSlot ls = a.lm_slot[slot];
    if (ls.model < 0) return;
    const LmDesc d = a.lm_desc[ls.model];
    int s = a.lm_state[slot];
    if ((unsigned)s >= (unsigned)d.n_nodes) s = d.start;      // a state read from memory is range-checked before it indexes anything
    const int V = a.n_valid;
    float *cell = reinterpret_cast<float *>(lds);
    unsigned short *next = reinterpret_cast<unsigned short *>(lds + (size_t)V * 4);
    lr.bias = br.bonus != nullptr;
    // (a lane combines into the cells it filled itself, n = tid + 256 j: no barrier between the fill and the walk)
    if (!lr.bias) for (int n = threadIdx.x; n < V; n += 256) { cell[n] = __uint_as_float(kBiasNoEdge); next[n] = 0; }
    for (int n = threadIdx.x; n < V; n += 256) {
        if (n == a.blank) continue;                            // the blank gets none
        const float c = cell[n];
        if (bias_forbidden(c)) continue;                       // a token forbidden by a strict set stays forbidden
        int sn = s;
        const float term = ls.w * lm_walk(d, sn, n) + ls.b;
        cell[n] = __float_as_uint(c) == kBiasNoEdge ? term : c + term;
    }
    __syncthreads();
    br.bonus = cell; br.next = next;
    lr.model = ls.model; lr.state = s;
}

// thread 0, after the decision: a non-blank decision moves the node along the token's text; the silence branch returns to the model's
// start node whether or not the context was cleared
__device__ __forceinline__ void lm_row_end(const DecideArgs &a, const LmRow &lr, int slot, bool is_blank, int tok, bool silence)
{
    const LmDesc d = a.lm_desc[lr.model];
    int s = lr.state;
    if (!is_blank) (void)lm_walk(d, s, tok);
    else if (silence) s = d.start;
    a.lm_state[slot] = s;
}
