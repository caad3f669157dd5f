"""Strict bias sets ("closed phrase lists") as DESIGN.md section 13 states them, in Python and numpy float32.  Written from the text of
the contract, not from csrc/bias.cc.  Text model, phrase normalisation, refusals, the unspellable-phrase rule, the byte trie and
best(node) are those of tests/bias_ref.py (whose BiasRef is asked first, so that the two cannot drift apart); what is new here:

    terminal(s)   some phrase ends at node s
    own edge      (s, n) -> s' as in section 13: the text of token n walked whole inside the trie from s, bonus best(s')
    live(s)       terminal(s), or some own edge of s leads to a live state                       (iterated to the fixed point)
    kept edge     an own edge whose target is live
    permitted(s)  the kept edges of s; at the root and at terminal states also the root's kept edges, for the tokens s has no kept
                  edge of its own for (the next phrase may begin where one ended).  Every other token is FORBIDDEN at s.
    lost phrase   its end cannot be reached from the root over permitted edges: counted with the unspellable ones
    refused       no phrase left

The search of a strict session takes the arg-max over the permitted tokens only; the blank is always permitted and never biased.
"""
import numpy as np

import bias_ref as R

STRICT = 1


class StrictRef:
    """texts: the token list as bytes.  phrases: [(bytes or str, boost)].  The interface of bias_ref.BiasRef (S, dropped, eff, csr,
    next, biased), so that bias_ref.Search and the replay of tests/bias_worker.py take either."""

    def __init__(self, texts, blank, phrases):
        texts = [R.as_bytes(t) for t in texts]
        base = R.BiasRef(texts, blank, phrases)                # the refusals of section 13, and its count of unspellable phrases
        kept = []
        for p, b in phrases:
            p = R.as_bytes(p)
            if p[:1] != b" ":
                p = b" " + p
            if R.segmentations(p, texts, blank):
                kept.append((p, np.float32(b)))
        child, best, ends = [dict()], [None], []
        for p, b in kept:
            node = 0
            for c in p:
                if c not in child[node]:
                    child[node][c] = len(child)
                    child.append(dict())
                    best.append(b)
                node = child[node][c]
                if b > best[node]:
                    best[node] = b
            ends.append(node)
        self.S = len(child)
        assert self.S == base.S
        self.terminal = set(ends)

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

        owns = [own(s) for s in range(self.S)]
        live = set(self.terminal)
        changed = True
        while changed:                                         # the fixed point, without relying on the numbering of the nodes
            changed = False
            for s in range(self.S):
                if s not in live and any(t in live for t, _ in owns[s].values()):
                    live.add(s)
                    changed = True
        keep = [{n: e for n, e in owns[s].items() if e[0] in live} for s in range(self.S)]
        self.eff = []
        for s in range(self.S):
            e = dict(keep[0]) if (s == 0 or s in self.terminal) else {}
            e.update(keep[s])
            self.eff.append(e)
        if sum(len(e) for e in self.eff) > R.MAX_EDGES:
            raise R.Refused("more than 4 M edges")
        reach, todo = {0}, [0]
        while todo:
            s = todo.pop()
            for t, _ in self.eff[s].values():
                if t not in reach:
                    reach.add(t)
                    todo.append(t)
        self.reachable = reach
        lost = sum(1 for e in ends if e not in reach)
        self.dropped = base.dropped + lost
        if len(kept) - lost == 0:
            raise R.Refused("no phrase left")
        for s in reach:
            assert self.eff[s], "a reachable state of a strict set has a permitted token"
        self.blank = blank
        self.flags = STRICT

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

    def permitted(self, s):
        """the non-blank tokens permitted at s, ascending"""
        return sorted(self.eff[s])

    def biased(self, v, s):
        """The row the search of a strict session compares: ONE fp32 addition for the permitted tokens, the blank untouched, and
        NaN for the forbidden ones -- `v > best` is false for a NaN, so bias_ref.argmax_record leaves them out exactly as it leaves
        out the blank.  (Which cells are forbidden is permitted(s), not the NaNs: the network may produce NaNs of its own.)"""
        v = np.asarray(v, np.float32)
        out = np.full(v.shape, np.nan, np.float32)
        out[self.blank] = v[self.blank]
        for n, (_, b) in self.eff[s].items():
            out[n] = np.float32(v[n] + np.float32(b))
        return out


def confidence(ref, v, s, k):
    """Section 12 over the blank and the permitted tokens only, in float64: (lse64, alt ids, alt logits as fp32 bits of v', n_alt).
    No permitted logit above the search's initial value: (nan, [], [], 0)."""
    vp = ref.biased(v, s)
    ids = [n for n in ref.permitted(s) if not np.isnan(vp[n])]
    if not ids or not (vp[ids] > R.INIT).any():
        return float("nan"), [], np.zeros(0, np.float32), 0
    order = sorted(ids, key=lambda n: (-float(vp[n]), n))[:k]
    terms = np.array([vp[n] for n in ref.permitted(s)] + [vp[ref.blank]], np.float64)      # forbidden terms are skipped, not added as zero
    m = np.nanmax(terms)
    lse = m + np.log(np.exp(terms - m).sum())
    return float(lse), order, vp[order], min(k, len(ids))
