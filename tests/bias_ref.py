"""Phrase boosting as DESIGN.md section 13 states it, in Python and numpy float32: the byte trie, the effective token edges of
every state, the biased logits v' and the state update.  Written from the text of the contract, not from the C++; the builder
(aprilx_bias_create), the host state machine's copy of the state and the decision kernel are checked against it.
"""
import numpy as np

MAX_STATES = 65535
MAX_EDGES = 4 << 20
MAX_PHRASE = 256
MAX_BOOST = 100.0
INIT = np.float32(-9999999999.0)


def as_bytes(x):
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


class Refused(ValueError):
    pass


def segmentations(phrase, texts, blank, limit=1000):
    """number of token sequences (non-blank, non-empty tokens) whose text is exactly `phrase` (with its leading blank)"""
    p = as_bytes(phrase)
    ways = [0] * (len(p) + 1)
    ways[0] = 1
    for i in range(len(p)):
        if ways[i]:
            for n, t in enumerate(texts):
                if n != blank and t and p.startswith(t, i):
                    ways[i + len(t)] = min(limit, ways[i + len(t)] + ways[i])
    return ways[len(p)]


class BiasRef:
    """texts: the token list as bytes.  phrases: [(bytes or str, boost)]."""

    def __init__(self, texts, blank, phrases):
        texts = [as_bytes(t) for t in texts]
        if not phrases:
            raise Refused("no phrases")
        kept = []
        self.dropped = 0
        for p, b in phrases:
            p = as_bytes(p)
            b = np.float32(b)
            if not p:
                raise Refused("empty phrase")
            if len(p) > MAX_PHRASE:
                raise Refused("phrase over 256 bytes")
            if not np.isfinite(b) or abs(float(b)) > MAX_BOOST:
                raise Refused("bad boost")
            if p[:1] != b" ":
                p = b" " + p
            if segmentations(p, texts, blank) == 0:            # nothing can spell it: left out, counted
                self.dropped += 1
                continue
            kept.append((p, b))
        # the byte trie; node 0 is the root, nodes are numbered as the phrases (in order) create them
        child = [dict()]
        best = [None]
        for p, b in kept:
            node = 0
            for c in p:
                if c not in child[node]:
                    if len(child) >= MAX_STATES:
                        raise Refused("more than 65535 states")
                    child[node][c] = len(child)
                    child.append(dict())
                    best.append(b)
                node = child[node][c]
                if b > best[node]:
                    best[node] = b
        self.S = len(child)

        def own(s):
            out = {}
            for n, t in enumerate(texts):
                if n == blank or not t:
                    continue
                node = s
                for c in t:
                    node = child[node].get(c, -1)
                    if node < 0:
                        break
                if node >= 0:
                    out[n] = (node, best[node])
            return out

        root = own(0)
        self.eff = []
        total = 0
        for s in range(self.S):
            e = dict(root)
            if s:
                e.update(own(s))
            self.eff.append(e)
            total += len(e)
            if total > MAX_EDGES:
                raise Refused("more than 4 M edges")
        self.blank = blank

    def csr(self):
        off = np.zeros(self.S + 1, np.int32)
        tok, nxt, bonus = [], [], []
        for s, e in enumerate(self.eff):
            for n in sorted(e):
                tok.append(n); nxt.append(e[n][0]); bonus.append(e[n][1])
            off[s + 1] = len(tok)
        return off, np.array(tok, np.int32), np.array(nxt, np.int32), np.array(bonus, np.float32)

    def next(self, s, tok):
        e = self.eff[s].get(int(tok))
        return e[0] if e else 0

    def biased(self, v, s):
        """v' of one row: ONE fp32 addition for the tokens with an effective edge from s, the other values untouched"""
        out = np.array(v, np.float32, copy=True)
        for n, (_, b) in self.eff[s].items():
            out[n] = np.float32(out[n] + np.float32(b))
        return out


def argmax_record(vp, blank):
    """(idx, max_val, blank_val) of the masked arg-max on one row: first maximum wins, the blank excluded, initial value -9999999999"""
    cand = np.where(np.isnan(vp), -np.inf, vp).astype(np.float32)          # `v > best` is false for a NaN
    cand[blank] = -np.inf
    bi = int(np.argmax(cand))                                              # the first maximum
    best = cand[bi]
    if not best > INIT:
        best, bi = INIT, -1
    return bi, np.float32(best), np.float32(vp[blank])


class Search:
    """decide_kernel's decision (the reference's src/april_session.c:322-429 as far as the next network call depends on
    it) with a bias state beside the search state.  cls: the token classes (bit 2 sentence end, 4 comma, 8 dot, 16 digit start)."""

    def __init__(self, cls, blank, ref=None):
        self.cls, self.blank, self.ref = cls, blank, ref
        self.ctx = [blank, blank]
        self.last_tok = -1
        self.last_emit = 0
        self.s = 0

    def step(self, v, early_emit, now):
        """one joiner evaluation with the network's logits v: returns (idx, max_val, blank_val, is_blank)"""
        vp = self.ref.biased(v, self.s) if self.ref is not None else np.asarray(v, np.float32)
        idx, mx, bl = argmax_record(vp, self.blank)
        return (idx, mx, bl, self.decide(idx, mx, bl, early_emit, now))

    def decide(self, idx, mx, bl, early_emit, now):
        tok, tv = idx, np.float32(mx)
        if tok < 0:
            tok, tv = (1 if self.blank == 0 else 0), INIT
        cleared = self.ctx[1] == self.blank
        same = self.ctx[1] == tok
        ee = np.float32(0.0 if same else early_emit)
        is_blank = bool(np.float32(bl - ee) > tv)
        tc = int(self.cls[tok])
        punct = (tc & 6) != 0
        if punct and self.last_tok >= 0 and (int(self.cls[self.last_tok]) & 16) and (tc & 8):
            punct = False
        if not cleared and punct and not same and tv > np.float32(bl - np.float32(3.5)):
            is_blank = False
        if not is_blank:
            self.last_emit = now
            self.ctx = [self.ctx[1], tok]
            self.last_tok = tok
            if self.ref is not None:
                self.s = self.ref.next(self.s, tok)
        elif ((now - self.last_emit) & 0xFFFFFFFF) >= 2200:
            self.last_tok = -1
            if self.ctx[0] != self.blank:
                self.ctx = [self.blank, self.blank]
            self.s = 0
        return is_blank

    def flush(self):
        self.last_tok = -1
        if self.ctx[0] != self.blank:
            self.ctx = [self.blank, self.blank]
        self.s = 0

    def state(self):
        return [self.ctx[0], self.ctx[1], self.last_tok, self.last_emit]


def token_classes(texts):
    out = np.zeros(len(texts), np.uint8)
    for i, t in enumerate(texts):
        t = as_bytes(t)
        f = 0
        if t[:1] == b" ": f |= 1
        if len(t) == 1 and t in (b".", b"!", b"?"): f |= 2
        if t == b",": f |= 4
        if t[:1] == b".": f |= 8
        if t[:1].isdigit(): f |= 16
        out[i] = f
    return out
