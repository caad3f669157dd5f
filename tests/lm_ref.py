"""The text-corpus language model as DESIGN.md section 20 states it, in Python and numpy: corpus normalisation, counts, interpolated
Witten-Bell in float64, the back-off automaton (the interchange form), the fp32 walk, and the fusion into the logit row.  Written from
the text of the contract, not from the C++; the builder (aprilx_lm_create), the host's walk (aprilx_lm_score_host), the host state
machine's copy of the node and the decision kernel's LM forms are checked against it.
"""
import math

import numpy as np

import search_options_ref as SO

f32 = np.float32
BOS = 0x0A
MIN_ORDER, MAX_ORDER, DEFAULT_ORDER = 2, 8, 5
MAX_CORPUS = 64 << 20
MAX_NODES = 4 << 20
MAX_ARCS = 16 << 20
MAX_VOCAB = 8192
MAX_WEIGHT, MAX_BONUS = 10.0, 100.0
INIT = SO.INIT


class Refused(ValueError):
    pass


def as_bytes(x):
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


def accepted(w, b):
    """the values aprilx_session_set_lm accepts"""
    return bool(np.isfinite(w)) and 0.0 <= w <= MAX_WEIGHT and bool(np.isfinite(b)) and abs(b) <= MAX_BONUS


def normalise(corpus, alphabet):
    """the kept lines (each with its prepended ' ') and the number of dropped ones"""
    kept, dropped = [], 0
    for raw in as_bytes(corpus).split(b"\n"):
        words = raw.replace(b"\r", b" ").replace(b"\t", b" ").split(b" ")
        words = [x for x in words if x]
        if not words:
            continue
        line = b" " + b" ".join(words)
        if any(c not in alphabet for c in line):
            dropped += 1
            continue
        kept.append(line)
    return kept, dropped


class LmRef:
    """texts: the token list as bytes (the blank included).  corpus: bytes or str."""

    def __init__(self, texts, blank, corpus, order=DEFAULT_ORDER):
        self.texts = [as_bytes(t) for t in texts]
        self.blank = blank
        if not MIN_ORDER <= order <= MAX_ORDER:
            raise Refused("order")
        if len(self.texts) > MAX_VOCAB:
            raise Refused("vocabulary")
        if len(as_bytes(corpus)) > MAX_CORPUS:
            raise Refused("corpus size")
        self.N = N = order
        self.alphabet = sorted({c for n, t in enumerate(self.texts) if n != blank for c in t})
        if BOS in self.alphabet:
            raise Refused("a token holds 0x0A")
        lines, self.dropped = normalise(corpus, set(self.alphabet))
        if not lines:
            raise Refused("no line left")
        # counts C(h, c)
        cnt = {}
        for line in lines:
            b = bytes([BOS]) + line
            m = len(b) - 1
            for i in range(1, m + 1):
                for k in range(0, min(N - 1, i) + 1):
                    d = cnt.setdefault(b[i - k:i], {})
                    d[b[i]] = d.get(b[i], 0) + 1
        # nodes: by length, then by bytes ascending; the root first
        self.ctx = sorted(cnt, key=lambda h: (len(h), h))
        assert self.ctx[0] == b""
        if len(self.ctx) > MAX_NODES:
            raise Refused("nodes")
        self.node = {h: i for i, h in enumerate(self.ctx)}
        self.cnt = cnt
        self.C = {h: sum(d.values()) for h, d in cnt.items()}
        self.T = {h: len(d) for h, d in cnt.items()}
        self.start = self.node[bytes([BOS])]
        A = len(self.alphabet)
        Te, Ce = self.T[b""], self.C[b""]
        self.unk_logp = f32(math.log(Te / ((Ce + Te) * A)))
        self._P = {}
        self.node_off = np.zeros(len(self.ctx) + 1, np.int32)
        back, bow, ab, al, an = [], [], [], [], []
        for i, h in enumerate(self.ctx):
            back.append(self.node[h[1:]] if h else 0)
            bow.append(f32(math.log(self.T[h] / (self.C[h] + self.T[h]))))
            for c in sorted(cnt[h]):
                ab.append(c)
                al.append(f32(math.log(self.P(c, h))))
                hc = (h + bytes([c]))[-(N - 1):]
                while hc not in self.node:
                    hc = hc[1:]
                an.append(self.node[hc])
            self.node_off[i + 1] = len(ab)
        if len(ab) > MAX_ARCS:
            raise Refused("arcs")
        self.back = np.array(back, np.int32)
        self.bow = np.array(bow, np.float32)
        self.arc_byte = np.array(ab, np.uint8)
        self.arc_logp = np.array(al, np.float32)
        self.arc_next = np.array(an, np.int32)
        self._arc = [{int(self.arc_byte[e]): e for e in range(self.node_off[s], self.node_off[s + 1])} for s in range(len(self.ctx))]

    def P(self, c, h):
        """P(c | h) in float64 for c in the alphabet and h a node's context (or any context: an unseen one backs off with weight 1)"""
        key = (c, h)
        if key in self._P:
            return self._P[key]
        if h == b"":
            A = len(self.alphabet)
            p = (self.cnt[b""].get(c, 0) + self.T[b""] / A) / (self.C[b""] + self.T[b""])
        elif h not in self.cnt:
            p = self.P(c, h[1:])
        else:
            p = (self.cnt[h].get(c, 0) + self.T[h] * self.P(c, h[1:])) / (self.C[h] + self.T[h])
        self._P[key] = p
        return p

    @property
    def nodes(self):
        return len(self.ctx)

    @property
    def arcs(self):
        return int(self.arc_byte.size)

    # ---- the walk: fp32, in the order written
    def step(self, s, c, acc):
        while True:
            e = self._arc[s].get(c)
            if e is not None:
                return int(self.arc_next[e]), f32(acc + self.arc_logp[e])
            if s == 0:
                return 0, f32(acc + self.unk_logp)
            acc = f32(acc + self.bow[s])
            s = int(self.back[s])

    def score(self, s, n):
        acc = f32(0.0)
        for c in self.texts[n]:
            s, acc = self.step(s, c, acc)
        return acc, s

    def next(self, s, n):
        return self.score(s, n)[1]

    # ---- fusion
    def term(self, s, n, w, b):
        return f32(f32(f32(w) * self.score(s, n)[0]) + f32(b))

    def fused(self, v, s, w, b, bias=None, bias_state=0):
        """The row the search of a session with a model compares: v'[n] = v[n] + cell, cell = term or bonus + term; the blank untouched;
        NaN for the tokens a strict set forbids (`v > best` is false for a NaN, as in tests/bias_strict_ref.py)."""
        v = np.asarray(v, np.float32)
        out = np.array(v, np.float32, copy=True)
        strict = bias is not None and getattr(bias, "flags", 0) & 1
        eff = bias.eff[bias_state] if bias is not None else {}
        for n in range(v.size):
            if n == self.blank:
                continue
            if strict and n not in eff:
                out[n] = np.nan
                continue
            cell = self.term(s, n, w, b)
            if n in eff:
                cell = f32(f32(eff[n][1]) + cell)
            out[n] = f32(v[n] + cell)
        return out

    def permitted(self, bias, bias_state):
        """the non-blank tokens that take part, ascending"""
        strict = bias is not None and getattr(bias, "flags", 0) & 1
        return sorted(bias.eff[bias_state]) if strict else [n for n in range(len(self.texts)) if n != self.blank]


class Row:
    """One slot's search with a model: the decision of section 14's statement (tests/search_options_ref.py) on the fused row, the node and
    the bias state beside the search state."""

    def __init__(self, cls, blank, lm=None, w=0.0, b=0.0, bias=None, opts=None):
        self.search = SO.Search(cls, blank, opts)
        self.lm, self.w, self.b, self.bias = lm, w, b, bias
        self.node = lm.start if lm is not None else 0
        self.trie = 0

    def compared(self, v):
        if self.lm is not None:
            return self.lm.fused(v, self.node, self.w, self.b, self.bias, self.trie)
        if self.bias is not None:
            return self.bias.biased(v, self.trie)
        return np.asarray(v, np.float32)

    def step(self, v, early_emit, now):
        """returns (idx, max_val, blank_val, is_blank, silence, ctx_changed); blank_val is the network's"""
        vp = self.compared(v)
        idx, mx, _ = SO.argmax_record(vp, self.search.blank)
        bl = f32(np.asarray(v, np.float32)[self.search.blank])
        is_blank, silence, changed = self.search.step(idx, mx, bl, early_emit, now)
        tok = idx if idx >= 0 else (1 if self.search.blank == 0 else 0)
        if not is_blank:
            if self.lm is not None:
                self.node = self.lm.next(self.node, tok)
            if self.bias is not None:
                self.trie = self.bias.next(self.trie, tok)
        elif silence:
            if self.lm is not None:
                self.node = self.lm.start
            self.trie = 0
        return idx, mx, bl, is_blank, silence, changed

    def flush(self):
        s = self.search
        s.last_tok = -1
        if s.ctx[0] != s.blank:
            s.ctx = [s.blank, s.blank]
        self.trie = 0
        if self.lm is not None:
            self.node = self.lm.start


def confidence(vp, ids, blank, k):
    """Section 12 over the blank and the tokens `ids` of the compared row vp, in float64: (lse64, alt ids, alt logits, n_alt)"""
    ids = [n for n in ids if not np.isnan(vp[n])]
    if not ids or not (vp[ids] > INIT).any():
        return float("nan"), [], np.zeros(0, np.float32), 0
    order = sorted(ids, key=lambda n: (-float(vp[n]), n))[:k]
    terms = np.array([vp[n] for n in ids] + [vp[blank]], np.float64)
    m = np.nanmax(terms)
    lse = m + np.log(np.exp(terms - m).sum())
    return float(lse), order, vp[order], min(k, len(ids))
