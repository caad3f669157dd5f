"""april_asr_amd -- host-side mirror of the reference's Python binding on top of the
MI355X-native libaprilasr.so.

Same public surface as `april_asr` (reference bindings/python/april_asr/_april.py:
Result :11-30, Token :32-57, Model :59-97, Session :110-179): `Model(path)`,
`Session(model, callback, asynchronous=False, no_rt=False, speaker_name="")`,
`session.feed_pcm16(bytes)`, `session.flush()`, `session.get_rt_speedup()`.
Extras that only make sense on a GPU engine are on `Model`/`SessionGroup`:
batched feeding of many sessions in one call, network-level parity entry points,
weight-blob export/import for the RCCL broadcast at load time.
"""
import ctypes as C
import math
import struct
import weakref
from enum import IntEnum
from typing import Callable, List, Sequence

import numpy as np

from . import _ffi

__all__ = ["Result", "Token", "Model", "Session", "SessionGroup", "Bias", "Lm", "lm_info", "VadEvent", "resampler_taps", "decode_host", "vad_plan", "vad_host", "vad_events_host",
           "DtmfEvent", "dtmf_plan", "dtmf_tables", "dtmf_host", "dtmf_decide_host", "dtmf_events_host",
           "ToneEvent", "tone_plan", "tone_tables", "tone_host", "tone_decide_host", "tone_events_host", "tone_name",
           "QualityEvent", "quality_plan", "quality_host", "quality_events_host",
           "snapshot_info"]


class Result(IntEnum):
    PARTIAL_RECOGNITION = 1   # text so far; the next call repeats it, updated
    FINAL_RECOGNITION = 2     # final; the next call starts from an empty list
    ERROR_CANT_KEEP_UP = 3    # asynchronous sessions: ingest ring overflowed, audio dropped
    SILENCE = 4               # some silence passed; empty token list


class VadEvent:
    """A voice-activity event of a session (Session(vad=...)): `kind` is VadEvent.SPEECH_START or VadEvent.SPEECH_END, `time_ms` the
    position in the session's audio on the frame clock."""
    SPEECH_START, SPEECH_END = 1, 2
    __slots__ = ("kind", "time_ms")

    def __init__(self, kind, time_ms):
        self.kind = int(kind)
        self.time_ms = int(time_ms)

    def __eq__(self, other):
        return isinstance(other, VadEvent) and (self.kind, self.time_ms) == (other.kind, other.time_ms)

    def __repr__(self):
        return "VadEvent(%s, %d)" % ("SPEECH_START" if self.kind == 1 else "SPEECH_END", self.time_ms)


class DtmfEvent:
    """A DTMF event of a session (Session(dtmf=...)): `kind` is DtmfEvent.DOWN or DtmfEvent.UP, `digit` one of "123A456B789C*0#D",
    `time_ms` the position in the session's audio on the frame clock."""
    DOWN, UP = 1, 2
    __slots__ = ("kind", "digit", "time_ms")

    def __init__(self, kind, digit, time_ms):
        self.kind = int(kind)
        self.digit = digit.decode("ascii") if isinstance(digit, bytes) else str(digit)
        self.time_ms = int(time_ms)

    def __eq__(self, other):
        return isinstance(other, DtmfEvent) and (self.kind, self.digit, self.time_ms) == (other.kind, other.digit, other.time_ms)

    def __repr__(self):
        return "DtmfEvent(%s, %r, %d)" % ("DOWN" if self.kind == 1 else "UP", self.digit, self.time_ms)


class QualityEvent:
    """A line-quality event of a session (Session(quality=...)): `kind` is QualityEvent.REPORT, CLIPPING_ON,
    CLIPPING_OFF, DROPOUT_ON or DROPOUT_OFF, `time_ms` the position in the session's audio on the frame clock.  A REPORT carries the
    integers of its interval -- frames, sum, sumsq, min, max, clip_samples, clipped_frames, dead_frames, quiet_sumsq, loud_sumsq -- ;
    `hop` is the samples per frame.  The levels in dB are derived from them in float64: rms_dbfs, peak_dbfs, dc, snr_db (None when a
    term is zero)."""
    REPORT, CLIPPING_ON, CLIPPING_OFF, DROPOUT_ON, DROPOUT_OFF = 1, 2, 3, 4, 5
    FIELDS = ("kind", "frames", "time_ms", "sum", "sumsq", "min", "max", "clip_samples", "clipped_frames", "dead_frames", "quiet_sumsq", "loud_sumsq", "hop")
    __slots__ = FIELDS

    def __init__(self, *values, **kw):
        for n in self.FIELDS:
            setattr(self, n, 0)
        for n, v in list(zip(self.FIELDS, values)) + list(kw.items()):
            setattr(self, n, int(v))

    @classmethod
    def from_struct(cls, e):
        return cls(*[getattr(e, n) for n in cls.FIELDS])

    def astuple(self):
        return tuple(getattr(self, n) for n in self.FIELDS)

    @property
    def rms_dbfs(self):
        n = self.frames * self.hop
        return 10.0 * math.log10(self.sumsq / float(n) / 32768.0 ** 2) if n and self.sumsq else None

    @property
    def peak_dbfs(self):
        peak = max(abs(self.min), abs(self.max))
        return 20.0 * math.log10(peak / 32768.0) if self.frames and peak else None

    @property
    def dc(self):
        n = self.frames * self.hop
        return self.sum / float(n) if n else None

    @property
    def snr_db(self):
        return 10.0 * math.log10(self.loud_sumsq / float(self.quiet_sumsq)) if self.loud_sumsq and self.quiet_sumsq else None

    def __eq__(self, other):
        return isinstance(other, QualityEvent) and self.astuple() == other.astuple()

    def __repr__(self):
        name = ("?", "REPORT", "CLIPPING_ON", "CLIPPING_OFF", "DROPOUT_ON", "DROPOUT_OFF")[self.kind if 0 < self.kind < 6 else 0]
        return "QualityEvent(%s, %d ms%s)" % (name, self.time_ms, ", %d frames" % self.frames if self.kind == 1 else "")


class ToneEvent:
    """A tone event of a session (Session(tones=...)): `kind` is ToneEvent.ON or ToneEvent.OFF, `f1_hz` and `f2_hz` the measured
    frequencies (a single tone: f2_hz == 0; a pair: f1_hz < f2_hz), `time_ms` the position in the session's audio on the frame clock
    (DESIGN.md section 18).  `name` is tone_name() of the frequencies: "dial", "busy", "cp425", "cng", "ced", "sit1".."sit3" or None."""
    ON, OFF = 1, 2
    __slots__ = ("kind", "f1_hz", "f2_hz", "time_ms")

    def __init__(self, kind, f1_hz, f2_hz, time_ms):
        self.kind, self.f1_hz, self.f2_hz, self.time_ms = int(kind), int(f1_hz), int(f2_hz), int(time_ms)

    @property
    def name(self):
        return tone_name(self.f1_hz, self.f2_hz)

    def __eq__(self, other):
        return isinstance(other, ToneEvent) and (self.kind, self.f1_hz, self.f2_hz, self.time_ms) == (other.kind, other.f1_hz, other.f2_hz, other.time_ms)

    def __repr__(self):
        return "ToneEvent(%s, %d, %d, %d)" % ("ON" if self.kind == 1 else "OFF", self.f1_hz, self.f2_hz, self.time_ms)


class Token:
    """One emitted token: text carries its own spacing; `logprob` is the raw joiner logit.

    Sessions created with `alternatives=K` (Session.set_confidence) also get `log_softmax` (the token's log-probability over the
    vocabulary of the joiner evaluation that produced it), `confidence` (= exp(log_softmax)), `blank_log_softmax` and
    `alternatives`: up to K (text, log_softmax) pairs by descending probability, the token itself first.  None otherwise."""
    __slots__ = ("token", "logprob", "word_boundary", "sentence_end", "time", "log_softmax", "confidence", "blank_log_softmax",
                 "alternatives")

    def __init__(self, raw, model=None):
        self.token = raw.token.decode("utf-8", "replace")
        self.logprob = float(raw.logprob)
        self.word_boundary = bool(raw.flags & 1)
        self.sentence_end = bool(raw.flags & 2)
        self.time = float(raw.time_ms) / 1000.0
        self.log_softmax = self.confidence = self.blank_log_softmax = self.alternatives = None
        if raw.reserved:
            info = C.cast(raw.reserved, C.POINTER(_ffi.AprilxTokenInfo)).contents
            self.log_softmax = float(info.token_logprob)
            self.confidence = math.exp(self.log_softmax) if self.log_softmax == self.log_softmax else float("nan")
            self.blank_log_softmax = float(info.blank_logprob)
            lse = np.float32(info.lse)
            self.alternatives = [(model.token(int(info.alt_id[i])) if model is not None else int(info.alt_id[i]),
                                  float(np.float32(info.alt_logit[i]) - lse)) for i in range(int(info.n_alt))]

    def __repr__(self):
        return "Token(%r, %.3f, wb=%d, eos=%d, t=%.2f)" % (self.token, self.logprob, self.word_boundary,
                                                             self.sentence_end, self.time)


class Model:
    def __init__(self, path: str = None, _handle=None):
        self._L = _ffi.init()
        if _handle is None:
            _handle = self._L.aam_create_model(path.encode("utf-8"))
        if not _handle:
            raise Exception("Failed to load model")
        self._handle = _handle
        d = _ffi.AprilxDims()
        self._L.aprilx_model_dims(self._handle, C.byref(d))
        self.dims = d

    # ---- reference surface
    def get_name(self) -> str:
        return self._L.aam_get_name(self._handle).decode("utf-8")

    def get_description(self) -> str:
        return self._L.aam_get_description(self._handle).decode("utf-8")

    def get_language(self) -> str:
        return self._L.aam_get_language(self._handle).decode("utf-8")

    def get_sample_rate(self) -> int:
        return int(self._L.aam_get_sample_rate(self._handle))

    def close(self):
        if getattr(self, "_handle", None):
            # sessions must not outlive their model (reference april_api.h:72-73): close the ones still open first, so a
            # session leaked by a failing caller cannot touch a freed model later (interpreter exit order is arbitrary)
            for s in list(getattr(self, "_sessions", ())):
                s.close()
            # ... and the ones the weak set no longer shows: when the model and its sessions become garbage together (sessions kept in
            # a reference cycle by their callbacks), the collector clears every weak reference before it runs any finalizer, and may
            # finalize the model first.  Their handles are kept as plain integers; Session.close() skips a session whose model is closed.
            for h in list(getattr(self, "_open_sessions", ())):
                self._L.aas_free(h)
            self._open_sessions = set()
            self._L.aam_free(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- engine-level extras
    def token(self, idx: int) -> str:
        t = self._L.aprilx_model_token(self._handle, idx)
        return t.decode("utf-8", "replace") if t is not None else ""

    def export_blob(self) -> np.ndarray:
        n = self._L.aprilx_model_blob_size(self._handle)
        buf = np.empty(n, np.uint8)
        if self._L.aprilx_model_export_blob(self._handle, buf.ctypes.data, n) != 0:
            raise RuntimeError("blob export failed")
        return buf

    @classmethod
    def load_host_only(cls, path: str):
        """Parse + extract + pack without any GPU object (loader / state-machine tests)."""
        L = _ffi.lib()
        h = L.aprilx_model_load_host(path.encode("utf-8"))
        if not h:
            raise Exception("Failed to load model")
        m = cls.__new__(cls)
        m._L = L; m._handle = h
        m.dims = _ffi.AprilxDims()
        L.aprilx_model_dims(h, C.byref(m.dims))
        return m

    def fbank_tables(self):
        n = self.dims.fft_size
        w = np.empty(n, np.float32); mel = np.empty((self.dims.mel, n // 2), np.float32)
        self._L.aprilx_model_fbank_tables(self._handle, w.ctypes.data, mel.ctypes.data)
        return w, mel

    @classmethod
    def from_blob(cls, blob, device_ptr: int = 0, size: int = 0, init_gpu: bool = True):
        """Build a model from an exported blob: a uint8 ndarray (host) or (device_ptr, size)."""
        L = _ffi.init() if (device_ptr or init_gpu) else _ffi.lib()
        if device_ptr:
            h = L.aprilx_model_from_blob(C.c_void_p(device_ptr), size, 1)
        else:
            blob = np.ascontiguousarray(blob, np.uint8)
            h = L.aprilx_model_from_blob(blob.ctypes.data, blob.size, 0)
        if not h:
            raise Exception("Failed to build model from blob")
        m = cls.__new__(cls)
        m._L = L; m._handle = h
        m.dims = _ffi.AprilxDims()
        L.aprilx_model_dims(h, C.byref(m.dims))
        return m

    # ---- one process per GPU: the model travels from rank 0 to the other ranks over RCCL inside the library
    @staticmethod
    def broadcast_id() -> bytes:
        """RCCL unique id (rank 0 creates it; hand the bytes to the other ranks by any means)."""
        L = _ffi.init()
        buf = C.create_string_buffer(128)
        n = L.aprilx_broadcast_get_id(buf, 128)
        if n <= 0:
            raise RuntimeError("aprilx_broadcast_get_id failed")
        return buf.raw[:n]

    @classmethod
    def broadcast(cls, root_model, rank: int, world: int, id_bytes: bytes):
        """Every rank calls this; rank 0 passes its model (and gets it back), the others pass None."""
        L = _ffi.init()
        idb = C.create_string_buffer(bytes(id_bytes), 128)
        h = L.aprilx_model_broadcast(root_model._handle if root_model is not None else None, rank, world, idb)
        if not h:
            raise Exception("model broadcast failed")
        if root_model is not None:
            return root_model
        m = cls.__new__(cls)
        m._L = L; m._handle = h
        m.dims = _ffi.AprilxDims()
        L.aprilx_model_dims(h, C.byref(m.dims))
        return m

    def load_info(self):
        info = _ffi.AprilxLoadInfo()
        self._L.aprilx_model_load_info(self._handle, C.byref(info))
        return info

    def save_blob(self, path: str, f16: bool = False):
        """Cache of the parsed + packed weights next to the model (aprilx_model_save_blob); f16: the half-size variant for
        fp16-operand mode (aprilx_model_save_blob_f16)."""
        fn = self._L.aprilx_model_save_blob_f16 if f16 else self._L.aprilx_model_save_blob
        if fn(self._handle, path.encode("utf-8")) != 0:
            raise RuntimeError("blob save failed")

    @classmethod
    def load_blob(cls, path: str, init_gpu: bool = True):
        L = _ffi.init() if init_gpu else _ffi.lib()
        h = L.aprilx_model_load_blob(path.encode("utf-8"))
        if not h:
            raise Exception("Failed to load model blob")
        m = cls.__new__(cls)
        m._L = L; m._handle = h
        m.dims = _ffi.AprilxDims()
        L.aprilx_model_dims(h, C.byref(m.dims))
        return m

    def run_encoder(self, x, h, c):
        d = self.dims
        x = np.ascontiguousarray(x, np.float32); n = x.shape[0]
        h = np.ascontiguousarray(h, np.float32).reshape(n, d.n_layers, d.d_model)
        c = np.ascontiguousarray(c, np.float32).reshape(n, d.n_layers, d.hidden)
        eout = np.empty((n, d.joiner), np.float32); h2 = np.empty_like(h); c2 = np.empty_like(c)
        rc = self._L.aprilx_run_encoder(self._handle, n, x.ctypes.data, h.ctypes.data, c.ctypes.data,
                                        eout.ctypes.data, h2.ctypes.data, c2.ctypes.data)
        assert rc == 0
        return eout, h2, c2

    def run_decoder(self, ctx):
        ctx = np.ascontiguousarray(ctx, np.int64).reshape(-1, self.dims.context)
        out = np.empty((ctx.shape[0], self.dims.joiner), np.float32)
        assert self._L.aprilx_run_decoder(self._handle, ctx.shape[0], ctx.ctypes.data, out.ctypes.data) == 0
        return out

    def run_joiner(self, eout, dout):
        e = np.ascontiguousarray(eout, np.float32).reshape(-1, self.dims.joiner)
        dd = np.ascontiguousarray(dout, np.float32).reshape(-1, self.dims.joiner)
        out = np.empty((e.shape[0], self.dims.vocab), np.float32)
        assert self._L.aprilx_run_joiner(self._handle, e.shape[0], e.ctypes.data, dd.ctypes.data, out.ctypes.data) == 0
        return out

    def run_fbank(self, pcm_frames):
        p = np.ascontiguousarray(pcm_frames, np.int16).reshape(-1, self.dims.fft_size)
        out = np.empty((p.shape[0], self.dims.mel), np.float32)
        assert self._L.aprilx_run_fbank(self._handle, p.shape[0], p.ctypes.data, out.ctypes.data) == 0
        return out

    def resample(self, pcm, in_rate: int) -> np.ndarray:
        """One whole segment of int16 PCM at `in_rate` converted to the model's rate by the device kernel (aprilx_resample; tests)."""
        a = np.ascontiguousarray(pcm, np.int16).ravel()
        lmk = np.zeros(3, np.int32)
        if self._L.aprilx_resampler_taps(int(in_rate), int(self.dims.sample_rate), lmk.ctypes.data, None, 0) != 0:
            raise ValueError("input rate %d is not accepted" % in_rate)
        cap = (a.size * int(lmk[0]) + int(lmk[1]) - 1) // int(lmk[1])
        out = np.zeros(max(cap, 1), np.int16)
        n = int(self._L.aprilx_resample(self._handle, int(in_rate), a.ctypes.data, a.size, out.ctypes.data, out.size))
        if n < 0:
            raise ValueError("aprilx_resample refused %d samples at %d Hz" % (a.size, in_rate))
        return out[:n]

    def decode(self, data, fmt) -> np.ndarray:
        """`data` (bytes or an array, taken as raw bytes) in the input format `fmt` -- (encoding, channels, channel), see
        Session.set_input_format -- decoded to int16 by the device kernel alone (aprilx_decode; tests)."""
        f = _input_format(*fmt)
        a = _raw_bytes(data)
        out = np.zeros(max(a.size, 1), np.int16)
        n = int(self._L.aprilx_decode(self._handle, C.byref(f), a.ctypes.data, a.size, out.ctypes.data, out.size))
        if n < 0:
            raise ValueError("aprilx_decode refused %d bytes of %r" % (a.size, (fmt,)))
        return out[:n]

    def decode_stats(self, device_index: int = 0):
        """(launches, frames, ms) of the decode launches of sessions with an input format (aprilx_model_decode_stats); ms under profile(1) only"""
        l, f, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
        if self._L.aprilx_model_decode_stats(self._handle, device_index, C.byref(l), C.byref(f), C.byref(ms)) != 0:
            raise ValueError("aprilx_model_decode_stats refused the call")
        return int(l.value), int(f.value), float(ms.value)

    def run_confidence(self, logits, k: int):
        """The side records of GIVEN logits rows [n][vocab] with k alternatives through the device code the search uses
        (aprilx_run_confidence; tests): an array of n _ffi.AprilxTokenInfo."""
        a = np.ascontiguousarray(logits, np.float32).reshape(-1, self.dims.vocab)
        out = (_ffi.AprilxTokenInfo * a.shape[0])()
        if self._L.aprilx_run_confidence(self._handle, a.shape[0], a.ctypes.data, int(k), out) != 0:
            raise ValueError("aprilx_run_confidence refused n=%d k=%d" % (a.shape[0], k))
        return out

    def bias(self, phrases, boost: float = 2.0, strict: bool = False):
        """A phrase-boosting set for this model (aprilx_bias_create_ex; no GPU needed): `phrases` is a list of strings / bytes, all with
        `boost` logit units, or of (phrase, boost) pairs.  Hand it to Session(..., bias=...) or Session.set_bias().
        `strict`: a closed phrase list -- the session emits only sequences of these phrases (APRILX_BIAS_STRICT)."""
        return Bias(self, phrases, boost, flags=BIAS_STRICT if strict else 0)

    def lm(self, text, order: int = 5):
        """A byte n-gram language model of `text` for this model's token list (aprilx_lm_create; no GPU needed):
        `text` is a str or bytes, one utterance per line, written the way the tokens are written.  Hand it to Session(..., lm=...) or
        Session.set_lm().  No accuracy is claimed for it: the default weight of a session is a placeholder until real audio has been run."""
        return Lm(self, text, order)

    def lm_stats(self, device_index: int = 0):
        """(decision launches of the language-model forms issued, models resident on the device, model uploads): all zero while no
        session of the engine has had a model (aprilx_model_lm_stats)"""
        a, b, c = C.c_uint64(0), C.c_int32(0), C.c_uint64(0)
        if self._L.aprilx_model_lm_stats(self._handle, int(device_index), C.byref(a), C.byref(b), C.byref(c)) != 0:
            raise ValueError("no such device")
        return int(a.value), int(b.value), int(c.value)

    def run_decide_lm(self, logits, early_emit, now_ms, rnd, state, lm, lm_state, weight, token_bonus, opts=None, bias=None, bias_state=None, op: int = 0):
        """One decision round on GIVEN logits rows with the language model on the rows whose lm_state is >= 0 (aprilx_run_decide_lm;
        tests); opts / bias as run_decide_opts.  Returns (records, search states [n][4], bias states [n] or None, nodes [n])."""
        st = np.ascontiguousarray(state, np.int32).reshape(-1, 4).copy()
        n = st.shape[0]
        lg = np.ascontiguousarray(logits, np.float32).reshape(n, self.dims.vocab)
        now = np.ascontiguousarray(now_ms, np.int32).reshape(n)
        bs = np.ascontiguousarray(bias_state, np.int32).reshape(n).copy() if bias is not None else None
        ls = np.ascontiguousarray(lm_state, np.int32).reshape(n).copy()
        arr = None
        if opts is not None:
            arr = (_ffi.AprilxSearchOptions * n)()
            for i, o in enumerate(opts):
                if o is not None:
                    arr[i].size = C.sizeof(_ffi.AprilxSearchOptions); arr[i].endpoint_silence_ms = int(o[0]); arr[i].blank_penalty = float(o[1])
        rec = np.zeros(n, np.dtype([("idx", np.int32), ("max", np.float32), ("blank", np.float32), ("flags", np.uint32)]))
        rc = self._L.aprilx_run_decide_lm(self._handle, n, int(op), lg.ctypes.data, float(early_emit), now.ctypes.data, int(rnd), st.ctypes.data,
                                          rec.ctypes.data, bias._handle if bias is not None else None, bs.ctypes.data if bs is not None else None,
                                          C.cast(arr, C.c_void_p) if arr is not None else None, lm._handle, ls.ctypes.data, float(weight), float(token_bonus))
        if rc != 0:
            raise ValueError("aprilx_run_decide_lm refused the call")
        return rec, st, bs, ls

    def run_confidence_lm(self, logits, k: int, lm, lm_state, weight, token_bonus, bias=None, bias_state=None):
        """run_confidence with the language model on the rows whose lm_state is >= 0 (aprilx_run_confidence_lm; tests)."""
        a = np.ascontiguousarray(logits, np.float32).reshape(-1, self.dims.vocab)
        ls = np.ascontiguousarray(lm_state, np.int32).reshape(a.shape[0])
        bs = np.ascontiguousarray(bias_state, np.int32).reshape(a.shape[0]) if bias is not None else None
        out = (_ffi.AprilxTokenInfo * a.shape[0])()
        if self._L.aprilx_run_confidence_lm(self._handle, a.shape[0], a.ctypes.data, int(k), bias._handle if bias is not None else None,
                                            bs.ctypes.data if bs is not None else None, lm._handle, ls.ctypes.data, float(weight), float(token_bonus), out) != 0:
            raise ValueError("aprilx_run_confidence_lm refused n=%d k=%d" % (a.shape[0], k))
        return out

    def run_confidence_biased(self, logits, k: int, bias, bias_state):
        """run_confidence with `bias` on the rows whose bias_state is >= 0 (aprilx_run_confidence_biased; tests)."""
        a = np.ascontiguousarray(logits, np.float32).reshape(-1, self.dims.vocab)
        bs = np.ascontiguousarray(bias_state, np.int32).reshape(a.shape[0])
        out = (_ffi.AprilxTokenInfo * a.shape[0])()
        if self._L.aprilx_run_confidence_biased(self._handle, a.shape[0], a.ctypes.data, int(k), bias._handle, bs.ctypes.data, out) != 0:
            raise ValueError("aprilx_run_confidence_biased refused n=%d k=%d" % (a.shape[0], k))
        return out

    def run_decide_biased(self, logits, early_emit, now_ms, rnd, state, bias, bias_state, op: int = 0):
        """One decision round on GIVEN logits rows with `bias` on the rows whose bias_state is >= 0 (aprilx_run_decide_biased; tests):
        returns (records [n] as (idx int32, max float32, blank float32, flags uint32), search states [n][4], bias states [n])."""
        st = np.ascontiguousarray(state, np.int32).reshape(-1, 4).copy()
        n = st.shape[0]
        lg = np.ascontiguousarray(logits, np.float32).reshape(n, self.dims.vocab)
        now = np.ascontiguousarray(now_ms, np.int32).reshape(n)
        bs = np.ascontiguousarray(bias_state, np.int32).reshape(n).copy()
        rec = np.zeros(n, np.dtype([("idx", np.int32), ("max", np.float32), ("blank", np.float32), ("flags", np.uint32)]))
        rc = self._L.aprilx_run_decide_biased(self._handle, n, int(op), lg.ctypes.data, float(early_emit), now.ctypes.data, int(rnd),
                                              st.ctypes.data, rec.ctypes.data, bias._handle, bs.ctypes.data)
        if rc != 0:
            raise ValueError("aprilx_run_decide_biased refused the call")
        return rec, st, bs

    def run_decide_opts(self, logits, early_emit, now_ms, rnd, state, opts, bias=None, bias_state=None, op: int = 0):
        """One decision round on GIVEN logits rows with per-row search options (aprilx_run_decide_opts; tests): `opts` has one entry per
        row, None (a row without options) or (endpoint_silence_ms, blank_penalty).  With `bias`, the set acts on the rows whose bias_state
        is >= 0.  Returns (records, search states [n][4], bias states [n] or None) as run_decide_biased."""
        st = np.ascontiguousarray(state, np.int32).reshape(-1, 4).copy()
        n = st.shape[0]
        lg = np.ascontiguousarray(logits, np.float32).reshape(n, self.dims.vocab)
        now = np.ascontiguousarray(now_ms, np.int32).reshape(n)
        bs = np.ascontiguousarray(bias_state, np.int32).reshape(n).copy() if bias is not None else None
        arr = (_ffi.AprilxSearchOptions * n)()
        for i, o in enumerate(opts):
            if o is not None:
                arr[i].size = C.sizeof(_ffi.AprilxSearchOptions); arr[i].endpoint_silence_ms = int(o[0]); arr[i].blank_penalty = float(o[1])
        rec = np.zeros(n, np.dtype([("idx", np.int32), ("max", np.float32), ("blank", np.float32), ("flags", np.uint32)]))
        rc = self._L.aprilx_run_decide_opts(self._handle, n, int(op), lg.ctypes.data, float(early_emit), now.ctypes.data, int(rnd), st.ctypes.data,
                                            rec.ctypes.data, bias._handle if bias is not None else None, bs.ctypes.data if bs is not None else None, arr)
        if rc != 0:
            raise ValueError("aprilx_run_decide_opts refused the call")
        return rec, st, bs

    def run_vad(self, options, rows_list, first_row=None, states=None):
        """vad_kernel alone (aprilx_run_vad; tests): run r with options[r] (dicts / None as Session.set_vad) over rows_list[r] [n][mel], all
        in ONE launch; first_row[r] places the run in its scratch ring of max(n) rows, states[r] (AprilxVadState) is the state the run starts
        from (None: reset).  Returns ([bytes], [energies], [states after the runs])."""
        k = len(rows_list)
        opts = (_ffi.AprilxVadOptions * k)(*[_vad_options(o) for o in options])
        n = np.array([len(r) for r in rows_list], np.int32)
        fr = np.zeros(k, np.int32) if first_row is None else np.ascontiguousarray(first_row, np.int32)
        rows = np.ascontiguousarray(np.concatenate([np.asarray(r, np.float32).reshape(len(r), -1) for r in rows_list]), np.float32)
        assert rows.shape[1] == self.dims.mel
        st = (_ffi.AprilxVadState * k)(*(states if states is not None else [vad_reset_state() for _ in range(k)]))
        b = np.zeros(int(n.sum()), np.uint8); e = np.zeros(int(n.sum()), np.float32)
        rc = self._L.aprilx_run_vad(self._handle, k, C.addressof(opts), n.ctypes.data, fr.ctypes.data, rows.ctypes.data, C.addressof(st), b.ctypes.data, e.ctypes.data)
        if rc != 0:
            raise ValueError("aprilx_run_vad refused its arguments")
        cuts = np.cumsum(n)[:-1]
        return np.split(b, cuts), np.split(e, cuts), [st[i] for i in range(k)]

    def run_dtmf(self, options, frames_list, powers: bool = True):
        """dtmf_kernel alone (aprilx_run_dtmf; tests): run r with options[r] (dicts / True as Session.set_dtmf) over frames_list[r]
        [n][fft_size] int16, all in ONE launch.  Returns ([codes], [powers [n][9]])."""
        k = len(frames_list)
        opts = (_ffi.AprilxDtmfOptions * k)(*[_dtmf_options(o) for o in options])
        n = np.array([len(f) for f in frames_list], np.int32)
        fr = np.ascontiguousarray(np.concatenate([np.asarray(f, np.int16).reshape(len(f), -1) for f in frames_list]), np.int16)
        codes = np.zeros(int(n.sum()), np.uint8); pw = np.zeros((int(n.sum()), 9), np.float32)
        if self._L.aprilx_run_dtmf(self._handle, C.addressof(opts), k, n.ctypes.data, fr.ctypes.data, codes.ctypes.data, pw.ctypes.data if powers else None) != 0:
            raise ValueError("aprilx_run_dtmf refused its arguments")
        cuts = np.cumsum(n)[:-1]
        return np.split(codes, cuts), np.split(pw, cuts)

    def run_dtmf_decide(self, options, powers9):
        """the kernel's decision alone on given rows [n][9] of P[0..8), E (aprilx_run_dtmf_decide; tests): codes [n]"""
        q = np.ascontiguousarray(powers9, np.float32).reshape(-1, 9)
        codes = np.zeros(len(q), np.uint8)
        if self._L.aprilx_run_dtmf_decide(self._handle, C.byref(_dtmf_options(options)), len(q), q.ctypes.data, codes.ctypes.data) != 0:
            raise ValueError("aprilx_run_dtmf_decide refused its arguments")
        return codes

    def run_tones(self, options, frames_list, powers: bool = True):
        """tone_kernel alone (aprilx_run_tones; tests): run r with options[r] (dicts / True as Session.set_tones) over frames_list[r]
        [n][fft_size] int16, all in ONE launch.  Returns ([records [n][2] uint16], [powers [n][F + 1]])."""
        k = len(frames_list)
        opts = (_ffi.AprilxToneOptions * k)(*[_tone_options(o) for o in options])
        n = np.array([len(f) for f in frames_list], np.int32)
        fr = np.ascontiguousarray(np.concatenate([np.asarray(f, np.int16).reshape(len(f), -1) for f in frames_list]), np.int16)
        plan = tone_plan(self.dims.sample_rate, self.dims.fft_size, max(1, self.dims.frame_shift * 1000 // self.dims.sample_rate), options[0])
        rec = np.zeros((int(n.sum()), 2), np.uint16); pw = np.zeros((int(n.sum()), plan.F + 1), np.float32)
        if self._L.aprilx_run_tones(self._handle, C.addressof(opts), k, n.ctypes.data, fr.ctypes.data, rec.ctypes.data, pw.ctypes.data if powers else None) != 0:
            raise ValueError("aprilx_run_tones refused its arguments")
        cuts = np.cumsum(n)[:-1]
        return np.split(rec, cuts), np.split(pw, cuts)

    def run_tone_decide(self, options, powers):
        """the kernel's decision alone on given rows [n][F + 1] of P[0..F), E (aprilx_run_tone_decide; tests): records [n][2] uint16"""
        q = np.ascontiguousarray(powers, np.float32)
        q = q.reshape(len(q), -1)
        rec = np.zeros((len(q), 2), np.uint16)
        if self._L.aprilx_run_tone_decide(self._handle, C.byref(_tone_options(options)), len(q), q.ctypes.data, rec.ctypes.data) != 0:
            raise ValueError("aprilx_run_tone_decide refused its arguments")
        return rec

    def run_quality(self, clip_levels, frames_list):
        """quality_kernel alone (aprilx_run_quality; tests): run r with clip level clip_levels[r] over frames_list[r] [n][fft_size] int16,
        all in ONE launch.  Returns [records [n][8] uint32]."""
        k = len(frames_list)
        lv = np.array([int(x) for x in clip_levels], np.int32)
        n = np.array([len(f) for f in frames_list], np.int32)
        fr = np.ascontiguousarray(np.concatenate([np.asarray(f, np.int16).reshape(len(f), -1) for f in frames_list]), np.int16)
        if len(lv) != k or fr.shape[1] != self.dims.fft_size:
            raise ValueError("run_quality: one clip level per run, frames of fft_size samples")
        rec = np.zeros((int(n.sum()), 8), np.uint32)
        if self._L.aprilx_run_quality(self._handle, lv.ctypes.data, k, n.ctypes.data, fr.ctypes.data, rec.ctypes.data) != 0:
            raise ValueError("aprilx_run_quality refused its arguments")
        return np.split(rec, np.cumsum(n)[:-1])

    def quality_stats(self, device_index: int = 0):
        """(launches, frames, ms): quality launches of one GPU's engine, the frames they covered, and (while profiling) the kernel's time"""
        return self._detector_stats(self._L.aprilx_model_quality_stats, device_index)

    def tone_stats(self, device_index: int = 0):
        """(launches, frames, ms): tone launches of one GPU's engine, the frames they covered, and (while profiling) the kernel's time"""
        return self._detector_stats(self._L.aprilx_model_tone_stats, device_index)

    def _detector_stats(self, entry, device_index):
        l, f, ms = C.c_uint64(0), C.c_uint64(0), C.c_double(0)
        if entry(self._handle, device_index, C.byref(l), C.byref(f), C.byref(ms)) != 0:
            raise ValueError("no such device")
        return int(l.value), int(f.value), float(ms.value)

    def dtmf_stats(self, device_index: int = 0):
        """(launches, frames, ms): DTMF launches of one GPU's engine, the frames they covered, and (while profiling) the kernel's time"""
        return self._detector_stats(self._L.aprilx_model_dtmf_stats, device_index)

    def vad_stats(self, device_index: int = 0):
        """(launches, frames, ms): VAD launches of one GPU's engine, the frames they covered, and (while profiling) the kernel's time"""
        return self._detector_stats(self._L.aprilx_model_vad_stats, device_index)

    def snapshot_stats(self, device_index: int = 0):
        """(gathers, scatters, gather_ms, scatter_ms): snapshot / restore launches of one GPU's engine and (while profiling) their kernel time"""
        g, s, gm, sm = C.c_uint64(0), C.c_uint64(0), C.c_double(0), C.c_double(0)
        if self._L.aprilx_model_snapshot_stats(self._handle, device_index, C.byref(g), C.byref(s), C.byref(gm), C.byref(sm)) != 0:
            raise ValueError("no such device")
        return int(g.value), int(s.value), float(gm.value), float(sm.value)

    def stats(self, device_index: int = 0):
        s = _ffi.AprilxStats()
        self._L.aprilx_model_stats(self._handle, device_index, C.byref(s))
        return s

    def ramp_stats(self, device_index: int = 0):
        """(ramp_hosted, ramp_eligible): feeds whose first macro steps ran inside the previous feed's last ones, and split feeds that could have been"""
        h, e = C.c_uint64(0), C.c_uint64(0)
        if self._L.aprilx_model_ramp_stats(self._handle, device_index, C.byref(h), C.byref(e)) != 0:
            raise ValueError("aprilx_model_ramp_stats refused the call")
        return int(h.value), int(e.value)

    def ramp_stats2(self, device_index: int = 0):
        """dict: hosted, eligible, headless (layer graphs launched without their head), settled_wait / settled_other (deferred layer graphs enqueued
        by the stepping thread's wait for a flight / by any other engine entry)"""
        out = (C.c_uint64 * 5)()
        if self._L.aprilx_model_ramp_stats2(self._handle, device_index, out) != 0:
            raise ValueError("aprilx_model_ramp_stats2 refused the call")
        return dict(zip(("hosted", "eligible", "headless", "settled_wait", "settled_other"), (int(v) for v in out)))

    def feed_latencies(self, device_index: int = 0, reset: bool = False) -> np.ndarray:
        """hand-over -> delivery latency (ms) of the last completed ticks of one GPU's stepping thread, oldest first"""
        n = int(self._L.aprilx_model_feed_latency(self._handle, device_index, None, 0, 0))
        out = np.zeros(n, np.float64)
        if n:
            n = int(self._L.aprilx_model_feed_latency(self._handle, device_index, out.ctypes.data, n, 1 if reset else 0))
        elif reset:
            self._L.aprilx_model_feed_latency(self._handle, device_index, None, 0, 1)
        return out[:n]

    def profile(self, enable):
        """True / 1: launches one by one with hipEvents around them (per-class times in stats().kernel_ms); 2: the gates clock (feeds run as
        always, the gates kernels time themselves; stats().gates_clock_* after the next profile(0)); False / 0: off"""
        self._L.aprilx_model_profile(self._handle, int(enable))


BIAS_STRICT = 1                                   # APRILX_BIAS_STRICT


class Bias:
    """A set of boosted phrases.  Sessions that use it keep it alive after close().
    `flags`: BIAS_STRICT for a closed phrase list; `edges()` of such a set are the tokens permitted at a state."""

    def __init__(self, model: Model, phrases, boost: float = 2.0, flags: int = 0):
        self._L = model._L
        items = [(p, boost) if isinstance(p, (str, bytes)) else (p[0], p[1]) for p in phrases]
        raw = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p, _ in items]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        boosts = (C.c_float * max(len(raw), 1))(*[float(b) for _, b in items])
        err = C.create_string_buffer(256)
        self._handle = self._L.aprilx_bias_create_ex(model._handle, len(raw), arr, boosts, int(flags), err, 256)
        self.message = err.value.decode("utf-8", "replace")          # a note about left-out phrases when the call succeeded
        if not self._handle:
            raise ValueError("bias set refused: " + self.message)
        st, ed = C.c_int32(0), C.c_int64(0)
        self.dropped = int(self._L.aprilx_bias_info(self._handle, C.byref(st), C.byref(ed)))
        self.states, self.n_edges = int(st.value), int(ed.value)
        self.flags = int(self._L.aprilx_bias_flags(self._handle))
        self.strict = bool(self.flags & BIAS_STRICT)

    def edges(self, state: int):
        """(token ids, next states, bonuses) of the effective edges of one trie state, token ids ascending"""
        n = int(self._L.aprilx_bias_edges(self._handle, int(state), None, None, None, 0))
        if n < 0:
            raise ValueError("no state %d" % state)
        tok = np.zeros(n, np.int32); nxt = np.zeros(n, np.int32); bonus = np.zeros(n, np.float32)
        if n:
            assert self._L.aprilx_bias_edges(self._handle, int(state), tok.ctypes.data, nxt.ctypes.data, bonus.ctypes.data, n) == n
        return tok, nxt, bonus

    def csr(self):
        """(state_off [S + 1], edge_tok, edge_next, edge_bonus) as the device receives them"""
        parts = [self.edges(s) for s in range(self.states)]
        off = np.zeros(self.states + 1, np.int32)
        off[1:] = np.cumsum([p[0].size for p in parts])
        return (off,) + tuple(np.concatenate([p[i] for p in parts]) if parts else np.zeros(0) for i in range(3))

    def close(self):
        if getattr(self, "_handle", None):
            self._L.aprilx_bias_free(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Lm:
    """A byte n-gram language model built from plain text.  Sessions that use it keep it alive after close()."""

    def __init__(self, model: Model, text, order: int = 5):
        self._L = model._L
        raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        err = C.create_string_buffer(256)
        self._handle = self._L.aprilx_lm_create(model._handle, raw, len(raw), int(order), err, 256)
        self.message = err.value.decode("utf-8", "replace")          # a note about dropped lines when the call succeeded
        if not self._handle:
            raise ValueError("language model refused: " + self.message)
        for k, v in lm_info(self).items():
            setattr(self, k, v)

    def arrays(self):
        """dict(node_off [nodes + 1], back, bow [nodes], arc_byte, arc_logp, arc_next [arcs], unk_logp) as the device receives them"""
        nn, na = self.nodes, self.arcs
        d = dict(node_off=np.zeros(nn + 1, np.int32), back=np.zeros(nn, np.int32), bow=np.zeros(nn, np.float32),
                 arc_byte=np.zeros(na, np.uint8), arc_logp=np.zeros(na, np.float32), arc_next=np.zeros(na, np.int32))
        unk = C.c_float(0)
        rc = self._L.aprilx_lm_arrays(self._handle, *[d[k].ctypes.data for k in ("node_off", "back", "bow", "arc_byte", "arc_logp", "arc_next")], C.byref(unk), nn, na)
        assert rc == 0
        d["unk_logp"] = np.float32(unk.value)
        return d

    def score(self, state: int, tok: int):
        """(score, next node) of the contract's walk on the host (aprilx_lm_score_host)"""
        sc, nx = C.c_float(0), C.c_int32(0)
        if self._L.aprilx_lm_score_host(self._handle, int(state), int(tok), C.byref(sc), C.byref(nx)) != 0:
            raise ValueError("no such node or token")
        return np.float32(sc.value), int(nx.value)

    def close(self):
        if getattr(self, "_handle", None):
            self._L.aprilx_lm_free(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lm_info(lm: "Lm"):
    """dict(order, nodes, arcs, start, alphabet, dropped_lines) of a language model (aprilx_lm_info)"""
    o, n, st, al, a = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
    dropped = int(lm._L.aprilx_lm_info(lm._handle, C.byref(o), C.byref(n), C.byref(a), C.byref(st), C.byref(al)))
    if dropped < 0:
        raise ValueError("no language model")
    return dict(order=int(o.value), nodes=int(n.value), arcs=int(a.value), start=int(st.value), alphabet=int(al.value), dropped_lines=dropped)


def _dispatch(userdata, result_type, count, tokens):
    sess = C.cast(userdata, C.py_object).value
    sess._on_result(result_type, count, tokens)


_HANDLER = _ffi.HANDLER(_dispatch)


def _dispatch_vad(userdata, kind, time_ms):
    sess = C.cast(userdata, C.py_object).value
    if sess.vad_callback is not None:
        sess.vad_callback(VadEvent(kind, time_ms))


_VAD_HANDLER = _ffi.VAD_HANDLER(_dispatch_vad)


def _dispatch_dtmf(userdata, kind, digit, time_ms):
    sess = C.cast(userdata, C.py_object).value
    if sess.dtmf_callback is not None:
        sess.dtmf_callback(DtmfEvent(kind, digit, time_ms))


_DTMF_HANDLER = _ffi.DTMF_HANDLER(_dispatch_dtmf)


def _dispatch_tone(userdata, kind, f1_hz, f2_hz, time_ms):
    sess = C.cast(userdata, C.py_object).value
    if sess.tone_callback is not None:
        sess.tone_callback(ToneEvent(kind, f1_hz, f2_hz, time_ms))


_TONE_HANDLER = _ffi.TONE_HANDLER(_dispatch_tone)


def _dispatch_quality(userdata, event):
    sess = C.cast(userdata, C.py_object).value
    if sess.quality_callback is not None:
        sess.quality_callback(QualityEvent.from_struct(event.contents))


_QUALITY_HANDLER = _ffi.QUALITY_HANDLER(_dispatch_quality)


class Session:
    def __init__(self, model: Model, callback: Callable[[Result, List[Token]], None], asynchronous: bool = False,
                 no_rt: bool = False, speaker_name: str = "", raw_events: bool = False, counters=None, input_sample_rate=None,
                 alternatives=None, bias=None, endpoint_silence_ms=None, blank_penalty=None, max_utterance_ms=None,
                 input_format=None, channels: int = 1, channel: int = 0, vad=None, vad_callback=None,
                 dtmf=None, dtmf_callback=None, tones=None, tone_callback=None, lm=None, lm_weight: float = 0.3, lm_token_bonus: float = 0.0,
                 quality=None, quality_callback=None):
        """`counters`: a uint64 ndarray of 6 entries; when given, results are only counted by a C handler inside the
        library (calls, partial, final, cant_keep_up, silence, tokens) and `callback` is never invoked.
        `input_sample_rate`: the rate of the PCM this session will receive (converted to the model's rate on the GPU); None: the
        model's rate.
        `alternatives`: K in 1..8: every delivered Token carries its log-softmax, the blank's and the K best candidates
        (set_confidence); None / 0: off.
        `bias`: a Bias (Model.bias): the search boosts the tokens that continue one of its phrases (set_bias); None: off.
        `endpoint_silence_ms`, `blank_penalty`, `max_utterance_ms`: the session's search options (set_search_options); all None: none.
        `lm`, `lm_weight`, `lm_token_bonus`: an Lm (Model.lm): the search adds lm_weight * log P(token text) + lm_token_bonus to every
        non-blank logit (set_lm); None: off.  The default weight is a placeholder: no accuracy has been measured.
        `input_format`, `channels`, `channel`: the format of the audio this session will receive (set_input_format): "mulaw", "alaw",
        "f32" or "s16", 1..8 interleaved channels, the channel to take or -1 for their downmix; None: mono PCM16.
        `vad`, `vad_callback`: True or a dict of options (set_vad) switches the voice-activity detector on; `vad_callback` receives one
        VadEvent per speech start / end, on the thread that delivers the session's results.
        `dtmf`, `dtmf_callback`: True or a dict of options (set_dtmf) switches the DTMF detector on; `dtmf_callback` receives one DtmfEvent
        per key down / key up, on the same thread.
        `tones`, `tone_callback`: True or a dict of options (set_tones) switches the tone detector on; `tone_callback` receives one ToneEvent
        per tone on / tone off, on the same thread.
        `quality`, `quality_callback`: True or a dict of options (set_quality) switches the line-quality observer on; `quality_callback`
        receives one QualityEvent per report and per clipping / dropout on / off, on the same thread."""
        self.dtmf_callback = dtmf_callback
        self.quality_callback = quality_callback
        self.tone_callback = tone_callback
        self._L = model._L
        self.vad_callback = vad_callback
        self.info_log = None      # tests: a list that receives (type, [the token's AprilxTokenInfo as bytes, or None]) per result
        self.model = model
        self.callback = callback
        self._raw = raw_events
        cfg = _ffi.AprilConfig()
        cfg.flags = (2 if no_rt else 1) if asynchronous else 0
        if speaker_name:
            cfg.speaker = _ffi.AprilSpeakerID.from_buffer_copy(struct.pack("@q", hash(speaker_name)) * 2)
        if counters is not None:
            self._counters = counters
            cfg.handler = C.cast(self._L.aprilx_counting_handler, _ffi.HANDLER)
            cfg.userdata = counters.ctypes.data
        else:
            cfg.handler = _HANDLER
            cfg.userdata = id(self)
        self._handle = self._L.aas_create_session(model._handle, cfg)
        if not self._handle:
            raise Exception("Failed to create session")
        if not hasattr(model, "_sessions"):
            model._sessions = weakref.WeakSet()
        model._sessions.add(self)
        if not hasattr(model, "_open_sessions"):
            model._open_sessions = set()
        model._open_sessions.add(self._handle)             # (Model.close(): what the weak set cannot show during garbage collection)
        if input_sample_rate is not None:
            self.set_input_rate(input_sample_rate)
        if input_format is not None:
            self.set_input_format(input_format, channels, channel)
        if alternatives:
            self.set_confidence(alternatives)
        if bias is not None:
            self.set_bias(bias)
        if lm is not None:
            self.set_lm(lm, lm_weight, lm_token_bonus)
        if endpoint_silence_ms is not None or blank_penalty is not None or max_utterance_ms is not None:
            self.set_search_options(endpoint_silence_ms, blank_penalty, max_utterance_ms)
        if vad:
            self.set_vad(vad)
        if dtmf:
            self.set_dtmf(dtmf)
        if tones:
            self.set_tones(tones)
        if quality:
            self.set_quality(quality)

    def set_quality(self, options=True, callback=None) -> None:
        """Line-quality reports and events for this session (aprilx_session_set_quality): True for the defaults, or
        a dict with any of clip_level (32124 for mu-law lines, 32256 for A-law), clip_run_min, clip_hold_ms, dropout_ms, report_ms;
        None / False switches it off.  `callback` replaces the session's quality_callback.  Allowed right after creation and after a
        completed flush; the machine and its counters start afresh."""
        if callback is not None:
            self.quality_callback = callback
        if not options:
            rc = self._L.aprilx_session_set_quality(self._handle, None, C.cast(None, _ffi.QUALITY_HANDLER), None)
        else:
            rc = self._L.aprilx_session_set_quality(self._handle, C.byref(_quality_options(options)), _QUALITY_HANDLER, id(self))
        if rc != 0:
            raise ValueError("quality options %r refused (a value out of range, or audio fed since the last flush)" % (options,))

    def quality(self):
        """None when the observer is off, else a dict: the options in force, hop, hold_frames, dropout_frames, report_frames, clipping,
        dropout (what is on after the last frame read), frames_seen, frames, clipped_frames, dead_frames, clip_samples, reports
        (aprilx_session_quality).  Waits for the session to be idle."""
        o, i = _ffi.AprilxQualityOptions(), _ffi.AprilxQualityInfo()
        if self._L.aprilx_session_quality(self._handle, C.byref(o), C.byref(i)) != 1:
            return None
        d = {n: int(getattr(o, n)) for n in _QUALITY_FIELDS}
        d.update({n: int(getattr(i, n)) for n, _ in _ffi.AprilxQualityInfo._fields_})
        return d

    def set_tones(self, options=True, callback=None) -> None:
        """Tone events for this session (aprilx_session_set_tones): True for the defaults, or a dict with any of
        min_level_dbfs, second_db, min_share, tol_hz, min_tone_ms, min_pause_ms; None / False switches it off.  `callback` replaces the
        session's tone_callback.  Allowed right after creation and after a completed flush; the machine and its counters start afresh."""
        if callback is not None:
            self.tone_callback = callback
        if not options:
            rc = self._L.aprilx_session_set_tones(self._handle, None, C.cast(None, _ffi.TONE_HANDLER), None)
        else:
            rc = self._L.aprilx_session_set_tones(self._handle, C.byref(_tone_options(options)), _TONE_HANDLER, id(self))
        if rc != 0:
            raise ValueError("tone options %r refused (a value out of range, a model the detector refuses, or audio fed since the last flush)" % (options,))

    def tone_info(self):
        """None when the detector is off, else a dict: the options, W, k_lo, F, on_frames, off_frames, frames_seen, tonal_frames, tones,
        held (the (f1_hz, f2_hz) held after the last frame, or None) (aprilx_session_tones).  Waits for the session to be idle."""
        o, i = _ffi.AprilxToneOptions(), _ffi.AprilxToneInfo()
        if self._L.aprilx_session_tones(self._handle, C.byref(o), C.byref(i)) != 1:
            return None
        d = {n: getattr(o, n) for n in _TONE_FIELDS}
        d.update({n: int(getattr(i, n)) for n in ("W", "k_lo", "F", "on_frames", "off_frames", "frames_seen", "tonal_frames", "tones")})
        d["held"] = (int(i.held_f1), int(i.held_f2)) if i.held_f1 else None
        return d

    def set_dtmf(self, options=True, callback=None) -> None:
        """DTMF digits for this session (aprilx_session_set_dtmf): True for the defaults, or a dict with any of
        min_level_dbfs, twist_hi_db, twist_lo_db, rel_peak_db, min_share, min_tone_ms, min_pause_ms; None / False switches it off.
        `callback` replaces the session's dtmf_callback.  Allowed right after creation and after a completed flush; the machine and
        its counters start afresh."""
        if callback is not None:
            self.dtmf_callback = callback
        if not options:
            rc = self._L.aprilx_session_set_dtmf(self._handle, None, C.cast(None, _ffi.DTMF_HANDLER), None)
        else:
            rc = self._L.aprilx_session_set_dtmf(self._handle, C.byref(_dtmf_options(options)), _DTMF_HANDLER, id(self))
        if rc != 0:
            raise ValueError("DTMF options %r refused (a value out of range, a model the detector refuses, or audio fed since the last flush)" % (options,))

    def dtmf_info(self):
        """None when the detector is off, else a dict: the options, Wd, on_frames, off_frames, frames_seen, tone_frames, digits, held (the
        digit held after the last frame, or "") (aprilx_session_dtmf).  Waits for the session to be idle."""
        o, i = _ffi.AprilxDtmfOptions(), _ffi.AprilxDtmfInfo()
        if self._L.aprilx_session_dtmf(self._handle, C.byref(o), C.byref(i)) != 1:
            return None
        d = {n: getattr(o, n) for n in _DTMF_FIELDS}
        d.update({n: int(getattr(i, n)) for n in ("Wd", "on_frames", "off_frames", "frames_seen", "tone_frames", "digits")})
        d["held"] = chr(i.held) if i.held else ""
        return d

    def set_vad(self, options=True, callback=None) -> None:
        """Voice activity for this session (aprilx_session_set_vad): True for the defaults, or a dict with any of
        band_lo_hz, band_hi_hz, onset_db, offset_db, onset_ms, hangover_ms, min_energy; None / False switches it off.  `callback`
        replaces the session's vad_callback.  Allowed right after creation and after a completed flush; the detector starts afresh."""
        if callback is not None:
            self.vad_callback = callback
        if not options:
            rc = self._L.aprilx_session_set_vad(self._handle, None, C.cast(None, _ffi.VAD_HANDLER), None)
        else:
            rc = self._L.aprilx_session_set_vad(self._handle, C.byref(_vad_options(options)), _VAD_HANDLER, id(self))
        if rc != 0:
            raise ValueError("voice-activity options %r refused (a value out of range, or audio fed since the last flush)" % (options,))

    def vad_info(self):
        """None when the detector is off, else a dict: the options, the band [b0, b1), onset_frames, hangover_frames, frames_seen,
        speech_frames, in_speech, segments (aprilx_session_vad).  Waits for the session to be idle."""
        o, i = _ffi.AprilxVadOptions(), _ffi.AprilxVadInfo()
        if self._L.aprilx_session_vad(self._handle, C.byref(o), C.byref(i)) != 1:
            return None
        d = {n: getattr(o, n) for n in _VAD_FIELDS}
        d.update({n: int(getattr(i, n)) for n in ("b0", "b1", "onset_frames", "hangover_frames", "frames_seen", "speech_frames", "in_speech", "segments")})
        return d

    def frames_seen(self) -> int:
        """real frames of the session since its creation (the frame clock of the voice-activity events)"""
        i = _ffi.AprilxVadInfo()
        self._L.aprilx_session_vad(self._handle, None, C.byref(i))
        return int(i.frames_seen)

    def _on_result(self, result_type, count, tokens):
        if self.info_log is not None:
            self.info_log.append((int(result_type), [C.string_at(tokens[i].reserved, C.sizeof(_ffi.AprilxTokenInfo)) if tokens[i].reserved
                                                     else None for i in range(count)]))
        if self._raw:
            # (type, [(token text, logprob, flags, time_ms)]) -- exact values, for parity tests
            self.callback(int(result_type), [(tokens[i].token, float(tokens[i].logprob), int(tokens[i].flags),
                                              int(tokens[i].time_ms)) for i in range(count)])
        else:
            self.callback(Result(result_type), [Token(tokens[i], self.model) for i in range(count)])

    def get_rt_speedup(self) -> float:
        return float(self._L.aas_realtime_get_speedup(self._handle))

    def feed_pcm16(self, data) -> None:
        """`data`: bytes of native-endian int16 mono samples (as the reference), or an int16 ndarray."""
        if isinstance(data, (bytes, bytearray, memoryview)):
            buf = (C.c_char * len(data)).from_buffer_copy(bytes(data))
            self._L.aas_feed_pcm16(self._handle, C.addressof(buf), len(data) // 2)
        else:
            a = np.ascontiguousarray(data, np.int16)
            self._L.aas_feed_pcm16(self._handle, a.ctypes.data, a.size)

    def feed(self, data) -> None:
        """Audio in the session's input format (aprilx_session_feed_bytes): bytes, or a uint8 / int16 / float32 array taken as its raw
        bytes.  A session without a format takes PCM16.  ValueError when `data` is not a whole number of frames (nothing is queued)."""
        a = _raw_bytes(data)
        if self._L.aprilx_session_feed_bytes(self._handle, a.ctypes.data, a.size) != 0:
            raise ValueError("%d bytes are not a whole number of the session's frames" % a.size)

    def flush(self) -> None:
        self._L.aas_flush(self._handle)

    def set_input_format(self, encoding="s16", channels: int = 1, channel: int = 0) -> None:
        """The audio fed from now on is `encoding` ("s16", "mulaw", "alaw", "f32", or the APRILX_ENC_* number) with `channels`
        interleaved channels, of which `channel` is taken (-1: their downmix); it is decoded on the GPU (aprilx_session_set_input_format,
        DESIGN.md section 15).  Allowed right after creation and after a completed flush; None or ("s16", 1, 0) restores mono PCM16."""
        if encoding is None:
            rc = self._L.aprilx_session_set_input_format(self._handle, None)
        else:
            rc = self._L.aprilx_session_set_input_format(self._handle, C.byref(_input_format(encoding, channels, channel)))
        if rc != 0:
            raise ValueError("input format %r refused (a value out of range, or audio fed since the last flush)" % ((encoding, channels, channel),))

    def input_format(self):
        """(encoding name, channels, channel) of the session, or None when it takes mono PCM16"""
        f = _ffi.AprilxInputFormat()
        if self._L.aprilx_session_input_format(self._handle, C.byref(f)) != 1:
            return None
        return _ENC_NAMES[int(f.encoding)], int(f.channels), int(f.channel)

    def set_input_rate(self, rate_hz: int) -> None:
        """The PCM fed from now on is at `rate_hz` (aprilx_session_set_input_rate): allowed right after creation and after a
        completed flush; the model's rate restores the default path."""
        if self._L.aprilx_session_set_input_rate(self._handle, int(rate_hz)) != 0:
            raise ValueError("input rate %d refused (outside 4000..384000 Hz / L > 4096, or audio fed since the last flush)" % rate_hz)

    def set_confidence(self, n_alternatives: int) -> None:
        """Tokens delivered from now on carry their log-softmax, the blank's and the `n_alternatives` (1..8) best candidates
        (aprilx_session_set_confidence); 0 switches it off.  Allowed right after creation and after a completed flush.  It changes
        no recognition result."""
        if self._L.aprilx_session_set_confidence(self._handle, int(n_alternatives)) != 0:
            raise ValueError("confidence with %d alternatives refused (0..8, and no audio fed since the last flush)" % n_alternatives)

    def set_bias(self, bias) -> None:
        """The search of this session uses the phrase-boosting set `bias` (Model.bias) from now on, starting at the root; None switches
        it off (aprilx_session_set_bias).  Allowed right after creation and after a completed flush."""
        if self._L.aprilx_session_set_bias(self._handle, bias._handle if bias is not None else None) != 0:
            raise ValueError("bias set refused (built for another token list, 64 sets in use on the engine already, or audio fed since the last flush)")

    def set_lm(self, lm, weight: float = 0.3, token_bonus: float = 0.0) -> None:
        """The search of this session uses the language model `lm` (Model.lm) from now on, starting at its start node; None switches it
        off (aprilx_session_set_lm).  weight: 0..10; token_bonus: |b| <= 100.  Allowed right after creation and after a completed flush.
        A session with a model cannot be snapshotted or restored into."""
        if self._L.aprilx_session_set_lm(self._handle, lm._handle if lm is not None else None, float(weight), float(token_bonus)) != 0:
            raise ValueError("language model refused (a value out of range, built for another token list, 8 models in use on the engine already, "
                             "or audio fed since the last flush)")

    def lm_state(self):
        """(host, device) node of the session's language model -- derived independently, must agree (tests)"""
        h, d = C.c_int32(0), C.c_int32(0)
        self._L.aprilx_session_lm_state(self._handle, C.byref(h), C.byref(d))
        return int(h.value), int(d.value)

    def set_search_options(self, endpoint_silence_ms=None, blank_penalty=None, max_utterance_ms=None) -> None:
        """The session's search options (aprilx_session_set_search_options): the silence after the last token that
        ends an utterance (200..60000 ms, default 2200), the constant subtracted from the blank logit in the decision (|p| <= 100, default
        0) and the cap on an utterance's length (0 = off, or 1000..600000 ms).  An argument left None takes its default; all three None
        returns the session to no options.  Allowed right after creation and after a completed flush; the options persist across flushes."""
        if endpoint_silence_ms is None and blank_penalty is None and max_utterance_ms is None:
            rc = self._L.aprilx_session_set_search_options(self._handle, None)
        else:
            o = _ffi.AprilxSearchOptions(C.sizeof(_ffi.AprilxSearchOptions), 2200 if endpoint_silence_ms is None else int(endpoint_silence_ms),
                                         0 if max_utterance_ms is None else int(max_utterance_ms), 0.0 if blank_penalty is None else float(blank_penalty))
            rc = self._L.aprilx_session_set_search_options(self._handle, C.byref(o))
        if rc != 0:
            raise ValueError("search options refused (a value out of range, or audio fed since the last flush)")

    @property
    def search_options(self):
        """(endpoint_silence_ms, blank_penalty, max_utterance_ms) of the session, or None when it has no options"""
        o = _ffi.AprilxSearchOptions()
        if self._L.aprilx_session_search_options(self._handle, C.byref(o)) != 1:
            return None
        return int(o.endpoint_silence_ms), float(o.blank_penalty), int(o.max_utterance_ms)

    def bias_state(self):
        """(host, device) trie state of the session's phrase boosting -- derived independently, must agree (tests)"""
        h, d = C.c_int32(0), C.c_int32(0)
        self._L.aprilx_session_bias_state(self._handle, C.byref(h), C.byref(d))
        return int(h.value), int(d.value)

    @property
    def alternatives(self) -> int:
        return int(self._L.aprilx_session_confidence(self._handle))

    @property
    def input_rate(self) -> int:
        return int(self._L.aprilx_session_input_rate(self._handle))

    def drain(self) -> None:
        """Asynchronous sessions: wait until everything queued so far was processed."""
        self._L.aprilx_session_drain(self._handle)

    def snapshot(self) -> bytes:
        """Everything dynamic the session holds, as a self-contained blob (aprilx_session_snapshot).  Waits until the
        session is idle and leaves it as it is: it may go on (a fork) or be closed (a move).  RuntimeError inside a flush or a handler."""
        n = int(self._L.aprilx_session_snapshot(self._handle, None, 0))
        if n < 0:
            raise RuntimeError("snapshot refused (a flush under way, or called from one of the session's handlers)")
        buf = (C.c_char * n)()
        got = int(self._L.aprilx_session_snapshot(self._handle, C.addressof(buf), n))
        if got < 0:
            raise RuntimeError("snapshot refused (the session changed between the two calls)")
        return bytes(buf[:got])

    def restore(self, blob) -> None:
        """Loads a snapshot into this FRESH session (aprilx_session_restore): same model and precision, configured as the source was
        (snapshot_info(blob) has the configuration).  From here on it continues the source's stream bit for bit.  ValueError with the
        library's reason when refused; the session stays usable."""
        b = bytes(blob)
        err = C.create_string_buffer(256)
        if self._L.aprilx_session_restore(self._handle, b, len(b), err, 256) != 0:
            raise ValueError("restore refused: %s" % err.value.decode(errors="replace"))

    def chunks(self) -> int:
        return int(self._L.aprilx_session_chunks(self._handle))

    def frames(self) -> np.ndarray:
        """every log-mel row the session's feature ring has received so far (real frames and flush padding), [rows][mel];
        parity tests of the online fbank"""
        total = int(self._L.aprilx_session_read_frames(self._handle, 0, 0, None))
        out = np.zeros((total, self.model.dims.mel), np.float32)
        if total:
            got = int(self._L.aprilx_session_read_frames(self._handle, 0, total, out.ctypes.data))
            if got == 2 ** 64 - 1:      # UINT64_MAX: the first rows have left the ring (more than ring_frames rows written)
                raise RuntimeError("frames(): %d rows written, the feature ring no longer holds the first ones" % total)
            if got != total:            # (a count: rows of the range were not written yet -- cannot happen for [0, total) on an idle session)
                raise RuntimeError("frames(): asked for %d rows, the session reports %d" % (total, got))
        return out

    def contexts(self):
        """(host context [2], device search state [ctx0, ctx1, last token, last emission ms]) -- derived independently, must agree"""
        h = np.zeros(2, np.int32); d = np.zeros(4, np.int32)
        self._L.aprilx_session_context(self._handle, h.ctypes.data, d.ctypes.data)
        return h, d

    def trace_logits(self, max_rows: int):
        self._trace = np.zeros((max_rows, self.model.dims.vocab), np.float32)
        self._trace_used = C.c_size_t(0)
        self._L.aprilx_session_trace_logits(self._handle, self._trace.ctypes.data, self._trace.size, C.byref(self._trace_used))

    def traced_logits(self):
        return self._trace[: self._trace_used.value // self.model.dims.vocab]

    def close(self):
        h = getattr(self, "_handle", None)
        if h:
            self._handle = None
            model = getattr(self, "model", None)
            # a model that has been closed has freed its sessions with it (Model.close()): the handle is dangling, leave it alone
            if model is not None and getattr(model, "_handle", None) is None:
                return
            if model is not None:
                getattr(model, "_open_sessions", set()).discard(h)
            self._L.aas_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SessionGroup:
    """Feeds many sessions in ONE library call so they advance in the same GPU steps."""

    def __init__(self, sessions: Sequence[Session]):
        self.sessions = list(sessions)
        self._L = self.sessions[0]._L
        n = len(self.sessions)
        self._handles = (C.c_void_p * n)(*[s._handle for s in self.sessions])
        self._ptrs = (C.c_void_p * n)()
        self._counts = (C.c_size_t * n)()

    def feed(self, pcm_list: Sequence[np.ndarray]):
        keep = []
        for i, p in enumerate(pcm_list):
            a = np.ascontiguousarray(p, np.int16)
            keep.append(a)
            self._ptrs[i] = a.ctypes.data
            self._counts[i] = a.size
        self._L.aprilx_feed_many(len(keep), self._handles, self._ptrs, self._counts)

    def plan(self, pcms: Sequence[np.ndarray], step_samples: int):
        """Pre-build the pointer/count arrays for feeding `step_samples` per session per call, so the
        per-step host cost is one library call (what a C/C++ host would do)."""
        n = len(self.sessions)
        self._plan_keep = [np.ascontiguousarray(p, np.int16) for p in pcms]
        steps = min(p.size for p in self._plan_keep) // step_samples
        self._plan = []
        for s in range(steps):
            ptrs = (C.c_void_p * n)(*[p.ctypes.data + 2 * s * step_samples for p in self._plan_keep])
            cnts = (C.c_size_t * n)(*([step_samples] * n))
            self._plan.append((ptrs, cnts))
        return steps

    def feed_planned(self, step: int):
        ptrs, cnts = self._plan[step]
        self._L.aprilx_feed_many(len(self.sessions), self._handles, ptrs, cnts)

    def feed_planned_pipelined(self, step: int, depth: int = 2):
        """Queue feed `step` of the plan and return once at most depth - 1 feeds per session are still open (depth 2: the
        library launches this feed behind the previous one and overlaps its host work with the GPU).  Call drain() at the end."""
        ptrs, cnts = self._plan[step]
        self._L.aprilx_feed_many_pipelined(len(self.sessions), self._handles, ptrs, cnts, depth)

    def feed_pipelined(self, pcm_list: Sequence[np.ndarray], depth: int = 2):
        keep = [np.ascontiguousarray(p, np.int16) for p in pcm_list]
        for i, a in enumerate(keep):
            self._ptrs[i] = a.ctypes.data
            self._counts[i] = a.size
        self._L.aprilx_feed_many_pipelined(len(keep), self._handles, self._ptrs, self._counts, depth)      # (samples are copied inside)

    def feed_bytes(self, data_list, depth: int = 0):
        """One buffer per session in that session's input format (aprilx_feed_many_bytes; a session without one takes PCM16): bytes or
        arrays taken as their raw bytes.  depth 0 blocks like feed(); depth >= 1 is the pipelined form (the bytes are copied; call
        drain() at the end).  ValueError when a buffer is not a whole number of its session's frames (nothing is queued)."""
        keep = [_raw_bytes(d) for d in data_list]
        for i, a in enumerate(keep):
            self._ptrs[i] = a.ctypes.data
            self._counts[i] = a.size
        if self._L.aprilx_feed_many_bytes(len(keep), self._handles, self._ptrs, self._counts, int(depth)) != 0:
            raise ValueError("a buffer is not a whole number of its session's frames")

    def feed_bytes_pipelined(self, data_list, depth: int = 2):
        self.feed_bytes(data_list, depth)

    def drain(self):
        self._L.aprilx_drain_many(len(self.sessions), self._handles)

    def flush(self):
        self._L.aprilx_flush_many(len(self.sessions), self._handles)

    def snapshot(self):
        """One blob per session (aprilx_snapshot_many): the device state of all sessions of an engine moves in ONE gather launch.
        RuntimeError when a session is refused."""
        n = len(self.sessions)
        sizes = (C.c_int64 * n)()
        if self._L.aprilx_snapshot_many(n, self._handles, None, None, sizes) != 0:
            raise RuntimeError("snapshot refused for sessions %r" % [i for i in range(n) if sizes[i] < 0])
        bufs = [(C.c_char * int(sizes[i]))() for i in range(n)]
        dsts = (C.c_void_p * n)(*[C.addressof(b) for b in bufs])
        caps = (C.c_size_t * n)(*[int(sizes[i]) for i in range(n)])
        if self._L.aprilx_snapshot_many(n, self._handles, dsts, caps, sizes) != 0:
            raise RuntimeError("snapshot refused for sessions %r" % [i for i in range(n) if sizes[i] < 0])
        return [bytes(bufs[i][:int(sizes[i])]) for i in range(n)]

    def restore(self, blobs):
        """blobs[i] into session i (aprilx_restore_many): one scatter launch per engine.  ValueError lists the sessions that were
        refused (the library logs each reason); the others have been restored."""
        n = len(self.sessions)
        keep = [bytes(b) for b in blobs]
        ptrs = (C.c_char_p * n)(*keep)
        sizes = (C.c_size_t * n)(*[len(b) for b in keep])
        status = (C.c_int * n)()
        if self._L.aprilx_restore_many(n, self._handles, ptrs, sizes, status) != 0:
            raise ValueError("restore refused for sessions %r" % [i for i in range(n) if status[i] != 0])


def snapshot_info(blob) -> dict:
    """The configuration, model identity and progress stored in a snapshot (aprilx_snapshot_info; no GPU, no model): enough to configure
    a receiving session from the blob alone -- `input_rate`, `input_format` ((encoding, channels, channel) or None), `alternatives`,
    `search_options` ((endpoint_silence_ms, blank_penalty, max_utterance_ms) or None), `vad` / `dtmf` / `tones` (option dicts or None),
    `bias` ({flags, states, edges, hash} or None: the set itself is the caller's to rebuild).  ValueError when the blob does not parse."""
    b = bytes(blob)
    i = _ffi.AprilxSnapshotInfo()
    if _ffi.lib().aprilx_snapshot_info(b, len(b), C.byref(i)) != 0:
        raise ValueError("not a snapshot, or a corrupt one")
    d = {n: int(getattr(i, n)) for n in ("version", "blob_size", "params_hash", "token_hash", "chunks", "frames_seen", "now_ms", "rows_written", "n_layers", "d_model",
                                         "hidden", "ffn", "joiner", "vocab", "mel", "segment_size", "segment_step", "sample_rate", "frame_shift_ms", "blank_id",
                                         "precision", "f16_tile", "input_rate", "ring_rows")}
    d["name"], d["description"] = i.name.decode(errors="replace"), i.description.decode(errors="replace")
    d["alternatives"] = int(i.confidence_k)
    d["input_format"] = (_ENC_NAMES[int(i.format.encoding)], int(i.format.channels), int(i.format.channel)) if i.has_format else None
    d["search_options"] = (int(i.search.endpoint_silence_ms), float(i.search.blank_penalty), int(i.search.max_utterance_ms)) if i.has_search_options else None
    d["vad"] = {n: getattr(i.vad, n) for n in _VAD_FIELDS} if i.has_vad else None
    d["dtmf"] = {n: getattr(i.dtmf, n) for n in _DTMF_FIELDS} if i.has_dtmf else None
    d["tones"] = {n: getattr(i.tones, n) for n in _TONE_FIELDS} if i.has_tones else None
    d["bias"] = dict(flags=int(i.bias_flags), states=int(i.bias_states), edges=int(i.bias_edges), hash=int(i.bias_hash)) if i.has_bias else None
    return d


ENCODINGS = {"s16": 0, "mulaw": 1, "alaw": 2, "f32": 3}      # APRILX_ENC_*
_ENC_NAMES = {v: k for k, v in ENCODINGS.items()}


_VAD_FIELDS = ("band_lo_hz", "band_hi_hz", "onset_db", "offset_db", "onset_ms", "hangover_ms", "min_energy")
_VAD_DEFAULTS = dict(band_lo_hz=200.0, band_hi_hz=4000.0, onset_db=5.0, offset_db=3.0, onset_ms=50, hangover_ms=300, min_energy=-12.0)


_DTMF_FIELDS = ("min_level_dbfs", "twist_hi_db", "twist_lo_db", "rel_peak_db", "min_share", "min_tone_ms", "min_pause_ms")
_DTMF_DEFAULTS = dict(min_level_dbfs=-40.0, twist_hi_db=4.0, twist_lo_db=8.0, rel_peak_db=8.0, min_share=0.6, min_tone_ms=20, min_pause_ms=20)


def _detector_options(options, struct, fields, defaults, what):
    """a detector's public options struct (size, `fields` in the struct's order, flags) from True / a dict over `defaults` / the struct itself"""
    if isinstance(options, struct):
        return options
    d = dict(defaults)
    if isinstance(options, dict):
        unknown = set(options) - set(fields)
        if unknown:
            raise ValueError("unknown %s options %r" % (what, sorted(unknown)))
        d.update(options)
    kinds = dict(struct._fields_)
    return struct(C.sizeof(struct), *[(float if kinds[n] is C.c_float else int)(d[n]) for n in fields], 0)


def _vad_options(options):
    return _detector_options(options, _ffi.AprilxVadOptions, _VAD_FIELDS, _VAD_DEFAULTS, "voice-activity")


def _dtmf_options(options):
    return _detector_options(options, _ffi.AprilxDtmfOptions, _DTMF_FIELDS, _DTMF_DEFAULTS, "DTMF")


_TONE_FIELDS = ("min_level_dbfs", "second_db", "min_share", "tol_hz", "min_tone_ms", "min_pause_ms")
_TONE_DEFAULTS = dict(min_level_dbfs=-40.0, second_db=10.0, min_share=0.7, tol_hz=20, min_tone_ms=60, min_pause_ms=30)


def _tone_options(options):
    return _detector_options(options, _ffi.AprilxToneOptions, _TONE_FIELDS, _TONE_DEFAULTS, "tone")


def tone_plan(sample_rate: int, fft_size: int, frame_shift_ms: int, options=True):
    """The detector's plan (AprilxTonePlan) of a model with this rate, fft size and frame shift, on the host (aprilx_tone_plan);
    ValueError when the options or the model are refused."""
    plan = _ffi.AprilxTonePlan()
    if _ffi.lib().aprilx_tone_plan(int(sample_rate), int(fft_size), int(frame_shift_ms), C.byref(_tone_options(options)), C.byref(plan)) != 0:
        raise ValueError("tone options %r refused" % (options,))
    return plan


def tone_tables(sample_rate: int, fft_size: int):
    """The detector's tables [2F][W] float32 (aprilx_tone_tables): row k cos, row F + k sin of bin k_lo + k"""
    plan = tone_plan(sample_rate, fft_size, 10)
    t = np.zeros((2 * plan.F, plan.W), np.float32)
    if _ffi.lib().aprilx_tone_tables(int(sample_rate), int(fft_size), t.ctypes.data, t.size) != t.size:
        raise ValueError("aprilx_tone_tables refused its arguments")
    return t


def tone_host(plan, tables, frames):
    """The contract on the host (aprilx_tone_host): frames [n][>= W] int16 -> (records [n][2] uint16, powers [n][F + 1] float32)"""
    f = np.ascontiguousarray(frames, np.int16)
    f = f.reshape(len(f), -1)
    t = np.ascontiguousarray(tables, np.float32)
    assert t.shape == (2 * plan.F, plan.W)
    rec = np.zeros((len(f), 2), np.uint16); pw = np.zeros((len(f), plan.F + 1), np.float32)
    if _ffi.lib().aprilx_tone_host(C.byref(plan), t.ctypes.data, len(f), f.ctypes.data, f.shape[1] if len(f) else plan.W, rec.ctypes.data, pw.ctypes.data) != 0:
        raise ValueError("aprilx_tone_host refused its arguments")
    return rec, pw


def tone_decide_host(plan, powers):
    """steps 3-7 on one row of P[0..F), E (aprilx_tone_decide_host): the record (f1_hz, f2_hz)"""
    q = np.ascontiguousarray(powers, np.float32)
    assert q.shape == (plan.F + 1,)
    r = int(_ffi.lib().aprilx_tone_decide_host(C.byref(plan), q.ctypes.data))
    if r < 0:
        raise ValueError("aprilx_tone_decide_host refused its arguments")
    return r & 0xffff, r >> 16


def tone_events_host(plan, frame_shift_ms: int, t0: int, records, machine=None, flush: bool = False):
    """The events that follow from the records [n][2] of frames [t0, t0 + n) (aprilx_tone_events_host) from `machine` (AprilxToneMachine,
    updated in place; None: idle); `flush`: a flush completes behind them.  Returns ([ToneEvent], machine)."""
    b = np.ascontiguousarray(records, np.uint16).reshape(-1, 2)
    cap = 2 * len(b) + 2              # (on_frames = off_frames = 1: a frame can give OFF and ON; a flush one more OFF)
    kinds = np.zeros(cap, np.int32); f1 = np.zeros(cap, np.uint32); f2 = np.zeros(cap, np.uint32); times = np.zeros(cap, np.uint64)
    m = machine if machine is not None else _ffi.AprilxToneMachine(0, 0, 0, 0, 0, 0)
    n = _ffi.lib().aprilx_tone_events_host(C.byref(plan), int(frame_shift_ms), int(t0), b.ctypes.data, len(b), 1 if flush else 0, C.byref(m),
                                           kinds.ctypes.data, f1.ctypes.data, f2.ctypes.data, times.ctypes.data, cap)
    if n < 0:
        raise ValueError("aprilx_tone_events_host refused its arguments")
    return [ToneEvent(kinds[i], f1[i], f2[i], times[i]) for i in range(n)], m


_QUALITY_FIELDS = ("clip_level", "clip_run_min", "clip_hold_ms", "dropout_ms", "report_ms")
_QUALITY_DEFAULTS = dict(clip_level=32767, clip_run_min=3, clip_hold_ms=1000, dropout_ms=200, report_ms=1000)


def _quality_options(options):
    """the public options struct (size, flags, then the fields) from True / a dict over the defaults / the struct itself"""
    if isinstance(options, _ffi.AprilxQualityOptions):
        return options
    d = dict(_QUALITY_DEFAULTS)
    if isinstance(options, dict):
        unknown = set(options) - set(_QUALITY_FIELDS)
        if unknown:
            raise ValueError("unknown quality options %r" % (sorted(unknown),))
        d.update(options)
    return _ffi.AprilxQualityOptions(C.sizeof(_ffi.AprilxQualityOptions), 0, *[int(d[n]) for n in _QUALITY_FIELDS])


def quality_plan(sample_rate: int, frame_samples: int, frame_shift_ms: int, options=True):
    """The observer's plan (AprilxQualityPlan) of a model with this rate, frame length in samples and frame shift, on the host
    (aprilx_quality_plan); ValueError when the options or the model are refused."""
    plan = _ffi.AprilxQualityPlan()
    if _ffi.lib().aprilx_quality_plan(int(sample_rate), int(frame_samples), int(frame_shift_ms), C.byref(_quality_options(options)), C.byref(plan)) != 0:
        raise ValueError("quality options %r refused" % (options,))
    return plan


def quality_host(hop: int, clip_level: int, frames):
    """The records on the host (aprilx_quality_host): frames [n][>= hop] int16 -> records [n][8] uint32"""
    f = np.ascontiguousarray(frames, np.int16)
    f = f.reshape(len(f), -1)
    rec = np.zeros((len(f), 8), np.uint32)
    if _ffi.lib().aprilx_quality_host(int(hop), int(clip_level), len(f), f.ctypes.data, f.shape[1] if len(f) else int(hop), rec.ctypes.data) != 0:
        raise ValueError("aprilx_quality_host refused its arguments")
    return rec


def quality_events_host(plan, frame_shift_ms: int, t0: int, records, machine=None, flush: bool = False):
    """The events that follow from the records [n][8] of frames [t0, t0 + n) (aprilx_quality_events_host) from `machine`
    (AprilxQualityMachine, updated in place; None: a fresh one); `flush`: a flush completes behind them.  Returns ([QualityEvent], machine)."""
    b = np.ascontiguousarray(records, np.uint32).reshape(-1, 8)
    cap = 3 * len(b) + 3              # (a frame gives at most one clipping event, one dropout event and a report; a flush two OFFs and a report)
    ev = (_ffi.AprilxQualityEvent * cap)()
    m = machine if machine is not None else _ffi.AprilxQualityMachine()
    n = _ffi.lib().aprilx_quality_events_host(C.byref(plan), int(frame_shift_ms), int(t0), b.ctypes.data, len(b), 1 if flush else 0, C.byref(m), C.addressof(ev), cap)
    if n < 0:
        raise ValueError("aprilx_quality_events_host refused its arguments")
    return [QualityEvent.from_struct(ev[i]) for i in range(n)], m


def tone_name(f1_hz: int, f2_hz: int = 0, tol_hz: int = 20):
    """"dial", "busy", "cp425", "cng", "ced", "sit1", "sit2", "sit3" or None (aprilx_tone_name)"""
    s = _ffi.lib().aprilx_tone_name(int(f1_hz), int(f2_hz), int(tol_hz))
    return s.decode() if s else None


def dtmf_plan(sample_rate: int, fft_size: int, frame_shift_ms: int, options=True):
    """The detector's plan (AprilxDtmfPlan) of a model with this rate, fft size and frame shift, on the host (aprilx_dtmf_plan);
    ValueError when the options or the model are refused."""
    plan = _ffi.AprilxDtmfPlan()
    if _ffi.lib().aprilx_dtmf_plan(int(sample_rate), int(fft_size), int(frame_shift_ms), C.byref(_dtmf_options(options)), C.byref(plan)) != 0:
        raise ValueError("DTMF options %r refused" % (options,))
    return plan


def dtmf_tables(sample_rate: int, Wd: int):
    """The detector's tables [16][Wd] float32 (aprilx_dtmf_tables): rows 0..7 cos, 8..15 sin of the eight frequencies"""
    t = np.zeros((16, int(Wd)), np.float32)
    if _ffi.lib().aprilx_dtmf_tables(int(sample_rate), int(Wd), t.ctypes.data, t.size) != t.size:
        raise ValueError("aprilx_dtmf_tables refused its arguments")
    return t


def dtmf_host(plan, tables, frames):
    """The contract on the host (aprilx_dtmf_host): frames [n][>= Wd] int16 -> (codes [n] uint8, powers [n][9] float32)"""
    f = np.ascontiguousarray(frames, np.int16)
    f = f.reshape(len(f), -1)
    t = np.ascontiguousarray(tables, np.float32)
    assert t.shape == (16, plan.Wd)
    codes = np.zeros(len(f), np.uint8); pw = np.zeros((len(f), 9), np.float32)
    if _ffi.lib().aprilx_dtmf_host(C.byref(plan), t.ctypes.data, len(f), f.ctypes.data, f.shape[1] if len(f) else plan.Wd, codes.ctypes.data, pw.ctypes.data) != 0:
        raise ValueError("aprilx_dtmf_host refused its arguments")
    return codes, pw


def dtmf_decide_host(plan, powers9) -> int:
    """steps 3-4 on one row of P[0..8), E (aprilx_dtmf_decide_host): the code"""
    q = np.ascontiguousarray(powers9, np.float32)
    assert q.shape == (9,)
    return int(_ffi.lib().aprilx_dtmf_decide_host(C.byref(plan), q.ctypes.data))


def dtmf_events_host(plan, frame_shift_ms: int, t0: int, codes, machine=None, flush: bool = False):
    """The events that follow from the codes of frames [t0, t0 + n) (aprilx_dtmf_events_host) from `machine` (AprilxDtmfMachine, updated
    in place; None: idle); `flush`: a flush completes behind them.  Returns ([DtmfEvent], machine)."""
    b = np.ascontiguousarray(codes, np.uint8)
    cap = 2 * len(b) + 2              # (on_frames = off_frames = 1: a frame can give UP and DOWN; a flush one more UP)
    kinds = np.zeros(cap, np.int32); digits = np.zeros(cap, np.uint8); times = np.zeros(cap, np.uint64)
    m = machine if machine is not None else _ffi.AprilxDtmfMachine(0, 0, 0)
    n = _ffi.lib().aprilx_dtmf_events_host(C.byref(plan), int(frame_shift_ms), int(t0), b.ctypes.data, len(b), 1 if flush else 0, C.byref(m),
                                           kinds.ctypes.data, digits.ctypes.data, times.ctypes.data, cap)
    if n < 0:
        raise ValueError("aprilx_dtmf_events_host refused its arguments")
    return [DtmfEvent(kinds[i], chr(digits[i]), times[i]) for i in range(n)], m


def vad_reset_state():
    """the detector's reset state (AprilxVadState)"""
    inf = float("inf")
    return _ffi.AprilxVadState(0.0, inf, (C.c_float * 8)(*([inf] * 8)), 0, 0, 0, 0, 1, 0)


def vad_plan(mel, sample_rate: int, frame_shift_ms: int, options=True):
    """The detector's plan (AprilxVadPlan) from a mel table [nbins][nfft_bins] (Model.fbank_tables) on the host (aprilx_vad_plan_tables);
    ValueError when the options are refused."""
    m = np.ascontiguousarray(mel, np.float32)
    plan = _ffi.AprilxVadPlan()
    if _ffi.lib().aprilx_vad_plan_tables(m.ctypes.data, m.shape[0], m.shape[1], int(sample_rate), int(frame_shift_ms), C.byref(_vad_options(options)),
                                         C.byref(plan)) != 0:
        raise ValueError("voice-activity options %r refused" % (options,))
    return plan


def vad_host(plan, rows, state=None):
    """The contract on the host (aprilx_vad_host): rows [n][nbins] through the detector from `state` (updated in place; None: reset).
    Returns (bytes [n] uint8, energies [n] float32, state)."""
    r = np.ascontiguousarray(rows, np.float32)
    r = r.reshape(len(r), -1)
    st = state if state is not None else vad_reset_state()
    b = np.zeros(len(r), np.uint8); e = np.zeros(len(r), np.float32)
    if _ffi.lib().aprilx_vad_host(C.byref(plan), len(r), r.shape[1] if len(r) else max(1, plan.b1), r.ctypes.data, C.byref(st), b.ctypes.data, e.ctypes.data) != 0:
        raise ValueError("aprilx_vad_host refused its arguments")
    return b, e, st


def vad_events_host(plan, frame_shift_ms: int, t0: int, data, last_bit: int = 0):
    """The events that follow from the bytes of frames [t0, t0 + n) (aprilx_vad_events_host): ([VadEvent], new last bit)"""
    b = np.ascontiguousarray(data, np.uint8)
    cap = len(b) + 1
    kinds = np.zeros(cap, np.int32); times = np.zeros(cap, np.uint64)
    last = C.c_int32(int(last_bit))
    n = _ffi.lib().aprilx_vad_events_host(C.byref(plan), int(frame_shift_ms), int(t0), b.ctypes.data, len(b), C.byref(last), kinds.ctypes.data,
                                          times.ctypes.data, cap)
    if n < 0:
        raise ValueError("aprilx_vad_events_host refused its arguments")
    return [VadEvent(kinds[i], times[i]) for i in range(n)], int(last.value)


def _input_format(encoding, channels=1, channel=0):
    enc = ENCODINGS[encoding] if isinstance(encoding, str) else int(encoding)
    return _ffi.AprilxInputFormat(C.sizeof(_ffi.AprilxInputFormat), enc, int(channels), int(channel))


def _raw_bytes(data) -> np.ndarray:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(data), np.uint8)
    if not isinstance(data, np.ndarray) or data.dtype not in (np.uint8, np.int16, np.float32):
        raise TypeError("raw audio must be bytes or a uint8, int16 or float32 array, not %r" % (getattr(data, "dtype", type(data)),))
    return np.ascontiguousarray(data).reshape(-1).view(np.uint8)


def decode_host(data, fmt) -> np.ndarray:
    """`data` in the input format `fmt` = (encoding, channels, channel) decoded to int16 by the contract in plain C++
    (aprilx_decode_host; no GPU)."""
    L = _ffi.lib()
    f = _input_format(*fmt)
    a = _raw_bytes(data)
    out = np.zeros(max(a.size, 1), np.int16)
    n = int(L.aprilx_decode_host(C.byref(f), a.ctypes.data, a.size, out.ctypes.data, out.size))
    if n < 0:
        raise ValueError("aprilx_decode_host refused %d bytes of %r" % (a.size, (fmt,)))
    return out[:n]


def resampler_taps(in_rate: int, out_rate: int):
    """(L, M, K, taps[L][2K] float32) of the conversion in_rate -> out_rate as the library runs it (aprilx_resampler_taps; no GPU)."""
    L = _ffi.lib()
    lmk = np.zeros(3, np.int32)
    if L.aprilx_resampler_taps(int(in_rate), int(out_rate), lmk.ctypes.data, None, 0) != 0:
        raise ValueError("conversion %d -> %d Hz is not accepted" % (in_rate, out_rate))
    l, m, k = (int(x) for x in lmk)
    taps = np.zeros((l, 2 * k), np.float32)
    if taps.size and L.aprilx_resampler_taps(int(in_rate), int(out_rate), lmk.ctypes.data, taps.ctypes.data, taps.size) != 0:
        raise RuntimeError("aprilx_resampler_taps failed")
    return l, m, k, taps
