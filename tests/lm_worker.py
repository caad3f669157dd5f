"""Helpers of tests/test_lm_cpu.py and tests/test_gpu_lm.py: corpora made of a model's own token texts, the
comparison of a built model with tests/lm_ref.py, and the host state machine (aprilx_greedy_*) with a model attached."""
import ctypes as C

import numpy as np

import lm_ref as R

ARRAYS = ("node_off", "back", "bow", "arc_byte", "arc_logp", "arc_next")


def texts_of(m):
    return [m._L.aprilx_model_token(m._handle, i) or b"" for i in range(m.dims.vocab)]


def token_lines(texts, blank, rng, n_lines, per_line=(2, 6), pool=None):
    """n_lines lines made of the model's own token texts: each starts with a word token (' ...') and goes on with any tokens of `pool`"""
    ids = [i for i, t in enumerate(texts) if i != blank and t and t != b"<blk>"] if pool is None else list(pool)
    words = [i for i in ids if texts[i][:1] == b" " and len(texts[i]) > 1]
    lines = []
    for _ in range(n_lines):
        k = int(rng.integers(per_line[0], per_line[1] + 1))
        seq = [int(rng.choice(words))] + [int(rng.choice(ids)) for _ in range(k - 1)]
        lines.append(b"".join(texts[i] for i in seq))
    return lines


def corpus_of(lines):
    return b"\n".join(line[1:] if line[:1] == b" " else line for line in lines) + b"\n"


def same_model(lm, ref):
    """every array of the interchange form, byte for byte"""
    assert (lm.order, lm.nodes, lm.arcs, lm.start, lm.alphabet, lm.dropped_lines) == (ref.N, ref.nodes, ref.arcs, ref.start, len(ref.alphabet), ref.dropped)
    got = lm.arrays()
    for k in ARRAYS:
        want = getattr(ref, k)
        assert got[k].dtype == want.dtype and got[k].tobytes() == want.tobytes(), k
    assert np.float32(got["unk_logp"]).tobytes() == np.float32(ref.unk_logp).tobytes()
    assert lm.start != 0


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


class ProductGreedy:
    """aprilx_greedy_* with a language model: only the node is looked at"""

    def __init__(self, model, lm=None, w=0.3, b=0.0):
        from april_asr_amd import _ffi
        self.L = _ffi.lib()
        self._h = _ffi.HANDLER(lambda ud, typ, count, toks: None)
        self.g = self.L.aprilx_greedy_create(model._handle, self._h, None)
        self.ctx = (C.c_int32 * 2)()
        if lm is not None:
            assert self.L.aprilx_greedy_set_lm(self.g, lm._handle, w, b) == 0

    def step(self, idx, mx, bl, early, now):
        return bool(self.L.aprilx_greedy_step(self.g, int(idx), float(mx), float(bl), float(early), int(now), self.ctx))

    def node(self):
        return int(self.L.aprilx_greedy_lm_state(self.g))

    def finish(self):
        self.L.aprilx_greedy_finish(self.g)

    def close(self):
        self.L.aprilx_greedy_free(self.g)
