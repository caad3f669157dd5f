"""Mutation test of the reference-based tests against the DEVICE's copy of the search decision (round 6).

csrc/kernels_misc.hip decide_kernel holds the part of aas_process_logits (src/april_session.c:306-429) that the NEXT network call
depends on -- arg-max with the lower id winning ties, blank / non-blank with the early-emit term, the punctuation override and the digit-dot
rule, the context push, the 2.2 s silence that clears the context -- a third transcription beside the oracle's and the host's.

Two lists of single edits, each compiled (hipcc on a private copy of kernels_misc.hip and of the two files it includes, kernels_bias.inc and
kernels_confidence.inc, one of the three edited; linked with the library's other objects into its own .so) and run on the GPU by a worker
process under APRIL_ASR_LIB:
  MUTANTS        lines every instantiation of decide_body shares, and the blank id's uses outside the loop: through aprilx_run_decide against
                 the hand-derived cases on a blank-0 model and on blank39, the NaN row, the ties inside one lane on blank255
                 (tests/device_decide_mutant_worker.py);
  OPTIN_MUTANTS  the opt-in lines -- bias_scan / bias_apply / bias_row_begin / bias_row_end, strict sets, the OPT lines, confidence_row --
                 through aprilx_run_decide_biased, aprilx_run_decide_opts, aprilx_run_confidence and aprilx_run_confidence_biased against
                 bias_ref, bias_strict_ref, search_options_ref and confidence_ref on blank39 and blank1050
                 (tests/device_optin_mutant_worker.py).
A mutant that passes every check SURVIVES; the GPU tests fail unless there are none.  A worker that ends by a signal or at its time limit
is NOT killed: the run stops there, starts no further mutant and fails naming it.

No mutant widens an index range, removes or weakens a bound that keeps the kernel inside its allocations, or lets a loop run without end:
the `(unsigned)t < (unsigned)V` scatter guard, the n_states clamp, `n < V` and the K loop's upper bound are never edited.  Every mutant
differs from the product only in the values it computes.

usage: python tests/mutate_device_decide.py [-v] [--optin]        (tests/test_gpu_decide.py runs both inside the gpu suite)
"""
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import threading
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "april_asr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
DEVFLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden", "-w", "-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
MISC, BIAS, CONF = "kernels_misc.hip", "kernels_bias.inc", "kernels_confidence.inc"
FILES = (MISC, BIAS, CONF)
WORKER_TIME_LIMIT = 300

MUTANTS = [
    ("tie_takes_the_higher_id", "const bool take = (oi >= 0) && (best_i < 0 || ov > best || (ov == best && oi < best_i));", "const bool take = (oi >= 0) && (best_i < 0 || ov > best || (ov == best && oi > best_i));"),
    ("cleared_tests_context0", "const bool cleared = st.ctx1 == a.blank;", "const bool cleared = st.ctx0 == a.blank;"),
    ("same_tests_context0", "const bool same = st.ctx1 == tok;", "const bool same = st.ctx0 == tok;"),
    ("same_keeps_early_emit", "const float ee = same ? 0.0f : a.early_emit;", "const float ee = a.early_emit;"),
    ("blank_test_not_strict", "bool is_blank = (bl - ee) > tv;", "bool is_blank = (bl - ee) >= tv;"),
    ("early_emit_added", "bool is_blank = (bl - ee) > tv;", "bool is_blank = (bl + ee) > tv;"),
    ("comma_is_no_punctuation", "bool punct = (tc & (TKC_SENT_END | TKC_COMMA)) != 0;", "bool punct = (tc & TKC_SENT_END) != 0;"),
    ("digit_rule_for_every_punctuation", "(a.tok_class[st.last_tok] & TKC_DIGIT_START) && (tc & TKC_DOT)) punct = false;", "(a.tok_class[st.last_tok] & TKC_DIGIT_START)) punct = false;"),
    ("digit_rule_dropped", "(a.tok_class[st.last_tok] & TKC_DIGIT_START) && (tc & TKC_DOT)) punct = false;", "(a.tok_class[st.last_tok] & TKC_DIGIT_START) && (tc & TKC_DOT)) punct = punct;"),
    ("override_margin_2_5", "tv > (bl - 3.5f)) is_blank = false;", "tv > (bl - 2.5f)) is_blank = false;"),
    ("override_margin_4_5", "tv > (bl - 3.5f)) is_blank = false;", "tv > (bl - 4.5f)) is_blank = false;"),
    ("override_not_strict", "tv > (bl - 3.5f)) is_blank = false;", "tv >= (bl - 3.5f)) is_blank = false;"),
    ("override_on_cleared_context", "if (!cleared && punct && !same && tv", "if (punct && !same && tv"),
    ("override_on_repeated_token", "if (!cleared && punct && !same && tv", "if (!cleared && punct && tv"),
    ("override_for_every_token", "if (!cleared && punct && !same && tv", "if (!cleared && !same && tv"),
    ("emission_time_not_recorded", "            st.last_emit_ms = now;\n", "            ;\n"),
    ("context_not_shifted", "st.ctx0 = st.ctx1; st.ctx1 = tok;", "st.ctx1 = tok;"),
    ("last_token_not_recorded", "            st.last_tok = tok;\n", "            ;\n"),
    ("silence_after_more_than_2200", "if (now - st.last_emit_ms >= 2200u) {", "if (now - st.last_emit_ms > 2200u) {"),
    ("silence_after_2100", "if (now - st.last_emit_ms >= 2200u) {", "if (now - st.last_emit_ms >= 2100u) {"),
    ("silence_after_2300", "if (now - st.last_emit_ms >= 2200u) {", "if (now - st.last_emit_ms >= 2300u) {"),
    ("silence_keeps_the_last_token", "                st.last_tok = -1;\n", "                ;\n"),
    ("clear_context_tests_context1", "if (st.ctx0 != a.blank) { st.ctx0 = a.blank; st.ctx1 = a.blank; rerun = true; }", "if (st.ctx1 != a.blank) { st.ctx0 = a.blank; st.ctx1 = a.blank; rerun = true; }"),
    # the arg-max loop itself: only a tie between two ids of ONE lane (n, n + 256) tells `>` from `>=` (blank255, V = 500)
    ("loop_tie_takes_the_higher_id_of_a_lane", "        else if (v > best) { best = v; best_i = n; }\n    }\n    // lowest index wins", "        else if (v >= best) { best = v; best_i = n; }\n    }\n    // lowest index wins"),
    # the blank id where the kernels carry it: each of these passes on every model whose blank is token 0
    ("blank_is_token_0_in_the_loop", "        if (n == a.blank) blank_v = v;\n        else if (v > best)", "        if (n == 0) blank_v = v;\n        else if (v > best)"),
    ("blank_logit_read_from_wave_0", "float bl = s_blank[(a.blank & 255) >> 6];", "float bl = s_blank[0];"),
    ("nan_fallback_is_always_token_1", "tok = a.blank == 0 ? 1 : 0;", "tok = 1;"),
    ("flush_clears_the_context_to_token_0", "if (st.ctx0 != a.blank) { st.ctx0 = a.blank; st.ctx1 = a.blank; }\n            a.state[slot] = st;", "if (st.ctx0 != a.blank) { st.ctx0 = 0; st.ctx1 = 0; }\n            a.state[slot] = st;"),
    # on blank39 token 0 is a digit-start token ("2"): the hand-derived digit-dot cases reach the rule with last_tok == 0
    ("digit_rule_last_token_from_1", "if (punct && st.last_tok >= 0 && (a.tok_class[st.last_tok] & TKC_DIGIT_START) && (tc & TKC_DOT)) punct = false;", "if (punct && st.last_tok >= 1 && (a.tok_class[st.last_tok] & TKC_DIGIT_START) && (tc & TKC_DOT)) punct = false;"),
    ("clear_context_half", "if (st.ctx0 != a.blank) { st.ctx0 = a.blank; st.ctx1 = a.blank; rerun = true; }", "if (st.ctx0 != a.blank) { st.ctx1 = a.blank; rerun = true; }"),
]
EQUIVALENT = [   # run on the blank-0 model alone
    # last_tok is -1 or the id of an emitted (non-blank) token; where the blank is token 0, `>= 0` and `>= 1` admit the same states (on blank39
    # token 0 is a digit-start token and the same edit is in MUTANTS)
    ("digit_rule_last_token_from_1", "if (punct && st.last_tok >= 0 && (a.tok_class[st.last_tok] & TKC_DIGIT_START) && (tc & TKC_DOT)) punct = false;", "if (punct && st.last_tok >= 1 && (a.tok_class[st.last_tok] & TKC_DIGIT_START) && (tc & TKC_DOT)) punct = false;"),
]



# ---------------------------------------------------------------- the opt-in lines: (name, file, original text, replacement)
OPTIN_MUTANTS = [
    # bias_scan: a COPY of decide_body's loop
    ("bias_scan_tie_takes_the_higher_id_of_a_lane", BIAS, "else if (v > best) { best = v; best_i = n; }", "else if (v >= best) { best = v; best_i = n; }"),
    ("bias_scan_compares_forbidden_tokens", BIAS, "else if (bias_forbidden(cell)) continue;", "else if (false) continue;"),
    # bias_apply
    ("bonus_subtracted", BIAS, "bias_forbidden(cell) ? v : v + cell;", "bias_forbidden(cell) ? v : v - cell;"),
    ("no_edge_cell_added", BIAS, "return __float_as_uint(cell) == kBiasNoEdge || bias_forbidden(cell) ? v : v + cell;", "return bias_forbidden(cell) ? v : v + cell;"),
    ("forbidden_cell_added", BIAS, "return __float_as_uint(cell) == kBiasNoEdge || bias_forbidden(cell) ? v : v + cell;", "return __float_as_uint(cell) == kBiasNoEdge ? v : v + cell;"),      # the blank's cell of a strict set makes the blank logit a NaN
    ("forbidden_is_the_no_edge_pattern", BIAS, "return __float_as_uint(cell) == kBiasForbidden; }", "return __float_as_uint(cell) == kBiasNoEdge; }"),
    # bias_row_begin (narrower edge ranges only; the scatter guard and the n_states clamp stay)
    ("first_edge_skipped", BIAS, "for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {", "for (int e = e0 + 1 + (int)threadIdx.x; e < e1; e += 256) {"),
    ("last_edge_skipped", BIAS, "for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {", "for (int e = e0 + (int)threadIdx.x; e < e1 - 1; e += 256) {"),
    ("strict_flag_inverted", BIAS, "(d.flags & 1) ? kBiasForbidden : kBiasNoEdge", "(d.flags & 1) ? kBiasNoEdge : kBiasForbidden"),
    ("next_state_stored_as_0", BIAS, "next[t] = (unsigned short)d.edge_next[e]; }", "next[t] = 0; }"),
    ("bonus_stored_as_0", BIAS, "{ bonus[t] = d.edge_bonus[e];", "{ bonus[t] = 0.0f;"),
    ("no_edge_leads_to_state_1", BIAS, "{ bonus[n] = fill; next[n] = 0; }", "{ bonus[n] = fill; next[n] = 1; }"),      # (a state the clamp of the next round admits or resets)
    # bias_row_end
    ("token_keeps_the_old_state", BIAS, "if (!is_blank) s = br.next[tok];", "if (!is_blank) s = br.state;"),
    ("silence_does_not_return_to_the_root", BIAS, "else if (silence) s = 0;", "else if (false) s = 0;"),
    ("every_blank_returns_to_the_root", BIAS, "else if (silence) s = 0;", "else if (true) s = 0;"),
    # the OPT lines of decide_body
    ("penalty_added", MISC, "if (so.endpoint_ms) bl = bl - so.blank_penalty; }", "if (so.endpoint_ms) bl = bl + so.blank_penalty; }"),
    ("own_endpoint_not_strict", MISC, "silence = now - st.last_emit_ms >= so.endpoint_ms;", "silence = now - st.last_emit_ms > so.endpoint_ms;"),
    ("own_endpoint_also_at_2200", MISC, "silence = now - st.last_emit_ms >= so.endpoint_ms;", "silence = now - st.last_emit_ms >= so.endpoint_ms || now - st.last_emit_ms >= 2200u;"),
    ("own_endpoint_ignored", MISC, "silence = now - st.last_emit_ms >= so.endpoint_ms;", "silence = now - st.last_emit_ms >= 2200u;"),
    ("trie_state_follows_2200_under_options", MISC, "OPT ? silence : is_blank && now - st.last_emit_ms >= 2200u);", "false ? silence : is_blank && now - st.last_emit_ms >= 2200u);"),
    # confidence_row: pass 1
    ("maximum_without_the_blank_registers", CONF, "const float v = c[j] = conf_logit(a, m, n, bonus);\n            mx = fmaxf(mx, v);", "const float v = c[j] = conf_logit(a, m, n, bonus);\n            if (n != a.blank) mx = fmaxf(mx, v);"),
    ("maximum_without_the_blank_re_evaluated", CONF, "const float v = conf_logit(a, m, n, bonus);\n        mx = fmaxf(mx, v);", "const float v = conf_logit(a, m, n, bonus);\n        if (n != a.blank) mx = fmaxf(mx, v);"),
    ("conf_tie_takes_the_higher_id_registers", CONF, "mx = fmaxf(mx, v);\n            if (n != a.blank && v > best) { best = v; best_i = n; }", "mx = fmaxf(mx, v);\n            if (n != a.blank && v >= best) { best = v; best_i = n; }"),
    ("conf_tie_takes_the_higher_id_re_evaluated", CONF, "mx = fmaxf(mx, v);\n        if (n != a.blank && v > best) { best = v; best_i = n; }", "mx = fmaxf(mx, v);\n        if (n != a.blank && v >= best) { best = v; best_i = n; }"),
    ("conf_arg_max_admits_the_blank", CONF, "mx = fmaxf(mx, v);\n            if (n != a.blank && v > best) { best = v; best_i = n; }", "mx = fmaxf(mx, v);\n            if (v > best) { best = v; best_i = n; }"),
    ("conf_skip_takes_the_blank_too", CONF, "return bonus && n != a.blank && bias_forbidden(bonus[n]);", "return bonus && bias_forbidden(bonus[n]);"),
    # pass 2
    ("sum_adds_forbidden_registers", CONF, "if (tid + 256 * j < V && !(skip >> j & 1)) sum += expf(c[j] - mx);", "if (tid + 256 * j < V) sum += expf(c[j] - mx);"),
    ("sum_adds_forbidden_re_evaluated", CONF, "if (!conf_skip(a, n, bonus)) sum += expf(conf_logit(a, m, n, bonus) - mx);", "if (true) sum += expf(conf_logit(a, m, n, bonus) - mx);"),
    ("sum_re_evaluates_the_last_register_too", CONF, "for (int n = tid + 256 * kConfRegs; n < V; n += 256)\n        if (!conf_skip(a, n, bonus)) sum", "for (int n = tid + 256 * (kConfRegs - 1); n < V; n += 256)\n        if (!conf_skip(a, n, bonus)) sum"),
    ("lse_subtracts_the_log", CONF, "out->lse = mx + logf(S);", "out->lse = mx - logf(S);"),
    # alternatives
    ("alternatives_offer_forbidden_registers", CONF, "if (tid + 256 * j < V && !(skip >> j & 1)) offer(c[j], tid + 256 * j);", "if (tid + 256 * j < V) offer(c[j], tid + 256 * j);"),
    ("alternatives_offer_forbidden_re_evaluated", CONF, "if (!conf_skip(a, n, bonus)) offer(conf_logit(a, m, n, bonus), n);", "if (true) offer(conf_logit(a, m, n, bonus), n);"),
    ("previous_pick_offered_again", CONF, "const bool after = v < pv || (v == pv && n > pi);", "const bool after = v < pv || (v == pv && n >= pi);"),
    ("wave_tie_takes_the_higher_id", CONF, "const int oi = __shfl_xor(i, off);\n        if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i)))", "const int oi = __shfl_xor(i, off);\n        if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi > i)))"),
    ("block_tie_takes_the_higher_id", CONF, "const int oi = s_i[phase][w];\n        if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i)))", "const int oi = s_i[phase][w];\n        if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi > i)))"),
    ("offer_tie_takes_the_higher_id_of_a_lane", CONF, "if (n != a.blank && after && (bi < 0 || v > bv)) { bv = v; bi = n; }", "if (n != a.blank && after && (bi < 0 || v >= bv)) { bv = v; bi = n; }"),
    ("offer_admits_the_blank", CONF, "if (n != a.blank && after && (bi < 0 || v > bv)) { bv = v; bi = n; }", "if (after && (bi < 0 || v > bv)) { bv = v; bi = n; }"),
    ("one_alternative_less_counted", CONF, "n_alt = k + 1;", "n_alt = k;"),
    ("nan_row_counts_an_alternative", CONF, "out->blank_val = conf_logit(a, m, a.blank, bonus); out->n_alt = 0;", "out->blank_val = conf_logit(a, m, a.blank, bonus); out->n_alt = 1;"),
]
OPTIN_EQUIVALENT = [   # (name, file, original, replacement, why no input tells them apart): each must SURVIVE
    ("one_register_per_lane", CONF, "constexpr int kConfRegs = 4;", "constexpr int kConfRegs = 1;",
     "the register path and the re-evaluated path compute the same expression: with one register all of n >= 256 is re-evaluated"),
    ("eight_registers_per_lane", CONF, "constexpr int kConfRegs = 4;", "constexpr int kConfRegs = 8;",
     "... and with eight, all of V = 1100 sits in registers: the two paths check each other"),
    ("blank_logit_of_bias_scan_without_the_bonus", BIAS, "if (n == a.blank) blank_v = v;", "if (n == a.blank) blank_v = raw;",
     "the blank has no edge (bias.cc leaves it out of the trie) and its cell of a strict set is never added: v == raw there"),
    ("side_record_blank_logit_without_the_bonus", CONF, "out->lse = mx + logf(S);\n        out->blank_val = conf_logit(a, m, a.blank, bonus);", "out->lse = mx + logf(S);\n        out->blank_val = conf_logit(a, m, a.blank, nullptr);",
     "the same: conf_logit adds nothing to the blank"),
    ("penalty_on_rows_without_options", MISC, "if (so.endpoint_ms) bl = bl - so.blank_penalty; }", "bl = bl - so.blank_penalty; }",
     "an entry without options is written as {0, 0.0f} by every path that writes one (Scheduler::set_search_options, Engine::free_slot, "
     "aprilx_run_decide_opts), and bl - 0.0f has bl's bits for every bl (tests/test_search_options_cpu.py)"),
    # (first listed as a mutant to kill: it survived, and no row can close it)
    ("unused_alternatives_name_token_0", CONF, "for (int k = n_alt; k < kConfMaxAlt; ++k) { out->alt_id[k] = -1; out->alt_logit[k] = 0.0f; }\n    }\n}", "for (int k = n_alt; k < kConfMaxAlt; ++k) { out->alt_id[k] = 0; out->alt_logit[k] = 0.0f; }\n    }\n}",
     "the host reads the first n_alt entries of a ConfRecord and fills the rest of an AprilxTokenInfo itself (session.cc fill_info, confidence_api.cc): "
     "the tail of the device record reaches no caller"),
    ("arg_max_re_evaluates_the_last_register_too", CONF, "for (int n = tid + 256 * kConfRegs; n < V; n += 256) {", "for (int n = tid + 256 * (kConfRegs - 1); n < V; n += 256) {",
     "a logit compared twice changes neither the maximum nor a strict `>` arg-max"),
    ("offers_re_evaluate_the_last_register_too", CONF, "for (int n = tid + 256 * kConfRegs; n < V; n += 256)\n            if (!conf_skip(a, n, bonus)) offer", "for (int n = tid + 256 * (kConfRegs - 1); n < V; n += 256)\n            if (!conf_skip(a, n, bonus)) offer",
     "a candidate offered twice: the second offer has v == bv and is not taken"),
]


def all_entries():
    """(name, file, original, replacement) of every mutant of both lists, equivalents included (tests/test_mutant_texts.py)"""
    out = [(n, MISC, o, r) for n, o, r in MUTANTS + EQUIVALENT]
    return out + [m[:4] for m in OPTIN_MUTANTS + OPTIN_EQUIVALENT]


def read_sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in FILES}


def build_variant(tmp, name, texts, objs):
    """a directory of its own per mutant: kernels_misc.hip and both .inc files, one of them edited (the quoted #include looks beside the
    including file first, so the copies win; everything else comes from -I csrc)"""
    d = os.path.join(tmp, name)
    os.makedirs(d)
    for f, text in texts.items():
        with open(os.path.join(d, f), "w") as fh:
            fh.write(text)
    obj = os.path.join(d, "kernels_misc.o")
    r = subprocess.run([HIPCC] + DEVFLAGS + ["-c", os.path.join(d, MISC), "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode:
        return None, r.stdout.decode()[-400:]
    so = os.path.join(d, "lib_" + name + ".so")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-Wl,--version-script=" + os.path.join(CSRC, "exports.map"), "-o", so] + objs + [obj, "-L/opt/rocm/lib", "-lrccl", "-lpthread"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode:
        return None, r.stdout.decode()[-400:]
    return so, ""


class Run:
    """one run of a list: the sources, the objects to link with, the worker's command line, and the flag that stops it"""

    def __init__(self, tmp, objs, worker, worker_args):
        self.tmp, self.objs, self.worker, self.worker_args = tmp, objs, worker, list(worker_args)
        self.src = read_sources()
        self.stop = threading.Event()
        self.aborted = []

    def mutant(self, name, fname, old, new, worker_args=None):
        """SURVIVED | KILLED | FAILED (did not build) | ABORTED (the worker ended by a signal or at its time limit) | SKIPPED (after an abort)"""
        if self.stop.is_set():
            return "SKIPPED", ""
        if self.src[fname].count(old) != 1:
            return "FAILED", "the text to mutate occurs %d times in %s" % (self.src[fname].count(old), fname)
        so, why = build_variant(self.tmp, name, dict(self.src, **{fname: self.src[fname].replace(old, new)}), self.objs)
        if so is None:
            return "FAILED", why
        if self.stop.is_set():
            return "SKIPPED", ""
        env = dict(os.environ, APRIL_ASR_LIB=so, APRIL_LOG_LEVEL="NONE")
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", self.worker)] + (self.worker_args if worker_args is None else list(worker_args)),
                               env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=WORKER_TIME_LIMIT)
        except subprocess.TimeoutExpired:
            self.stop.set()
            self.aborted.append((name, "the worker did not end within %d s" % WORKER_TIME_LIMIT))
            return "ABORTED", "time limit"
        finally:
            shutil.rmtree(os.path.join(self.tmp, name), ignore_errors=True)
        out = r.stdout.decode()
        if r.returncode < 0:
            self.stop.set()
            self.aborted.append((name, "the worker ended by signal %d: %s" % (-r.returncode, out.strip()[-200:])))
            return "ABORTED", "signal %d" % -r.returncode
        if r.returncode == 0 and "SURVIVED" in out:
            return "SURVIVED", ""
        return "KILLED", (out.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200]

    def check_not_aborted(self):
        assert not self.aborted, "the run stopped: %s (a worker that ends by a signal or at its time limit is not a killed mutant)" % self.aborted


def library_objects():
    objs = [o for o in sorted(glob.glob(os.path.join(CSRC, "build", "*.o"))) if os.path.basename(o) != "kernels_misc.o"]
    assert objs, "build the library first (csrc/build/*.o)"
    return objs


def write_models(tmp, names):
    sys.path.insert(0, ROOT)
    import blank_models as BM
    from april_asr_amd import synth_model as SM
    out = {}
    for n in names:
        if n == "tiny":
            out[n] = os.path.join(tmp, "tiny.april")
            SM.write_model(out[n], SM.TINY_DIMS)
        else:
            out[n] = BM.write(tmp, n)["path"]
    return out


def sort_results(res, verbose):
    killed, survivors, failures = [], [], []
    for name, status, why in res:
        if verbose:
            print("%-46s %s %s" % (name, status, why))
        if status in ("ABORTED", "SKIPPED"):
            continue
        (killed if status == "KILLED" else survivors if status == "SURVIVED" else failures).append((name, why))
    return killed, survivors, failures


def run_all(verbose=False, model_path=None, workers=6, blank39_path=None, ties_path=None):
    """the shared lines: returns (killed, survivors, equivalent_killed, build_failures).  model_path: a blank-0 model (the tiny one);
    blank39_path, ties_path: blank39 and a V >= 500 model (blank255); each is written when it is not given"""
    objs = library_objects()
    tmp = tempfile.mkdtemp(prefix="april_dmutants_")
    try:
        need = [n for n, p in (("tiny", model_path), ("blank39", blank39_path), ("blank255", ties_path)) if p is None]
        made = write_models(tmp, need)
        model_path, blank39_path, ties_path = model_path or made["tiny"], blank39_path or made["blank39"], ties_path or made["blank255"]
        run = Run(tmp, objs, "device_decide_mutant_worker.py", [model_path, blank39_path, ties_path])
        status, why = run.mutant("identity", MISC, "void launch_decide(", "void launch_decide(")
        assert status == "SURVIVED", "the unmutated device decision fails the checks through this harness: %s %s" % (status, why)
        with ThreadPoolExecutor(workers) as ex:
            res = list(ex.map(lambda m: (m[0],) + run.mutant(m[0], MISC, m[1], m[2]), MUTANTS))
            eqr = list(ex.map(lambda m: (m[0],) + run.mutant("eq_" + m[0], MISC, m[1], m[2], [model_path]), EQUIVALENT))
        run.check_not_aborted()
        killed, survivors, failures = sort_results(res, verbose)
        eq_killed = [(n, w) for n, st, w in eqr if st != "SURVIVED"]
        return killed, survivors, eq_killed, failures
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def run_optin(verbose=False, workers=6, blank39_path=None, blank1050_path=None):
    """the opt-in lines: returns (killed, survivors, equivalent_killed, build_failures)"""
    objs = library_objects()
    tmp = tempfile.mkdtemp(prefix="april_omutants_")
    try:
        made = write_models(tmp, [n for n, p in (("blank39", blank39_path), ("blank1050", blank1050_path)) if p is None])
        run = Run(tmp, objs, "device_optin_mutant_worker.py", [blank39_path or made["blank39"], blank1050_path or made["blank1050"]])
        status, why = run.mutant("identity", MISC, "void launch_decide(", "void launch_decide(")
        assert status == "SURVIVED", "the unmutated opt-in lines fail the checks through this harness: %s %s" % (status, why)
        with ThreadPoolExecutor(workers) as ex:
            res = list(ex.map(lambda m: (m[0],) + run.mutant(m[0], m[1], m[2], m[3]), OPTIN_MUTANTS))
            eqr = list(ex.map(lambda m: (m[0],) + run.mutant("eq_" + m[0], m[1], m[2], m[3]), OPTIN_EQUIVALENT))
        run.check_not_aborted()
        killed, survivors, failures = sort_results(res, verbose)
        eq_killed = [(n, w) for n, st, w in eqr if st != "SURVIVED"]
        return killed, survivors, eq_killed, failures
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    optin = "--optin" in sys.argv
    k, s, e, f = (run_optin if optin else run_all)(verbose="-v" in sys.argv)
    print("%d mutants of %s: %d killed, %d survived, %d failed to build; %d equivalent mutants, %d of them unexpectedly killed"
          % (len(OPTIN_MUTANTS if optin else MUTANTS), "the opt-in lines" if optin else "decide_kernel", len(k), len(s), len(f), len(OPTIN_EQUIVALENT if optin else EQUIVALENT), len(e)))
    for name, _ in s:
        print("SURVIVOR:", name)
    for name, why in e:
        print("EQUIVALENT KILLED:", name, why)
    for name, why in f:
        print("BUILD FAILURE:", name, why)
    sys.exit(1 if (s or e or f) else 0)
