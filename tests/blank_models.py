"""Models whose blank is not token 0, for the tests of the search decision (host, oracle and device).

The loader accepts any 0 <= blank_id < token_count, as the reference's params.c does, and the reference's exporter writes
sp.piece_to_id("<blk>"): a nonzero id is legal input.  All models here have the tiny dimensions except for the vocabulary and the
blank, so each is written and loaded in well under a second.

    name        V     blank   what it moves
    blank39     40    39      the last id; a hand-made token list with a digit-start token ("2") at id 0
    blank64     131   64      the first lane of wave 1
    blank255    500   255     the last lane of wave 3 (the `& 255` edge)
    blank256    500   256     lane 0, second stride
    blank1050   1100  1050    past the register window of confidence_row (kConfRegs * 256), wave 0

Test modules parametrise their existing tests over these names with `params()` (the ids the suite had stay as they were) and turn a
name into the dict the conftest fixtures return with `model_info()`.
"""
import os

import pytest

MODELS = {"blank39": (40, 39), "blank64": (131, 64), "blank255": (500, 255), "blank256": (500, 256), "blank1050": (1100, 1050)}
_written = {}


def hand_tokens_blank39():
    """the generated 40-entry list with "2" moved to id 0 and "<blk>" to id 39: every other token keeps its text.
    "2" and not " 1": the digit-dot rule looks at the FIRST byte of the last token's text (src/april_session.c:347), so " 1" is no
    digit-start token.  With "2" at id 0 the rule's `last_tok >= 0` is reached with last_tok == 0 by the hand-derived cases."""
    from april_asr_amd import synth_model as SM
    toks = SM.make_tokens(40)
    rest = [t for t in toks if t not in ("<blk>", "2")]
    out = ["2"] + rest + ["<blk>"]
    assert len(out) == 40 and sorted(out) == sorted(toks)
    return out


def write(model_dir, name):
    """write the model once per directory; returns dict(path, dims, weights, tokens, blank) as the conftest fixtures do"""
    from april_asr_amd import synth_model as SM
    path = os.path.join(str(model_dir), name + ".april")
    if path not in _written:
        V, blank = MODELS[name]
        # blank39 is also the model of the live sessions: with the generator's blank bias of 4.7 the blank wins every round of the
        # test audio and no token is ever delivered; with 3.0 tokens are, and the 2.2 s silence reset is reached after them
        extra = dict(tokens=hand_tokens_blank39(), blank_bias=3.0) if name == "blank39" else {}
        dims, w, toks = SM.write_model(path, dict(SM.TINY_DIMS, vocab=V), blank_id=blank, **extra)
        assert toks[blank] == "<blk>" and toks.count("<blk>") == 1
        _written[path] = dict(path=path, dims=dims, weights=w, tokens=toks, blank=blank)
    return _written[path]


def model_info(which, request):
    """`which`: a name of MODELS, or of a conftest fixture without its `_model` suffix"""
    if which in MODELS:
        request.getfixturevalue("built")
        return write(request.getfixturevalue("model_dir"), which)
    info = dict(request.getfixturevalue(which + "_model"))
    info.setdefault("blank", 0)
    return info


def params(values, ids, extra, base="tiny"):
    """pytest parameters (value, which): every value on `base` under the id it always had, then on the models of `extra`
    -- a list of names, or of (name, values) to run only some values there -- under '<id>-<name>'"""
    values, ids = list(values), [str(i) for i in ids]
    out = [pytest.param(v, base, id=i) for v, i in zip(values, ids)]
    for e in extra:
        name, some = (e, values) if isinstance(e, str) else e
        out += [pytest.param(v, name, id="%s-%s" % (ids[values.index(v)], name)) for v in some]
    return out
