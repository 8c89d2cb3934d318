"""Host side of beam search (no GPU): ``tests/beam_ref.py`` pinned against the installed transformers' ``_beam_search``, the C
ABI's new names, and the plumbing of ``generate(num_beams=n)`` through ``LlamaForCausalLM`` on the stand-in engine of
``test_fork_cpu.py``."""
import functools
import itertools
import math
import os

import pytest
import torch

import beam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- beam_ref == transformers ------------------------------------------------------------------------------------------------------
BEAMS = (1, 2, 3, 4)
SETTINGS = ((1.0, False), (0.0, "never"), (2.0, True))
STOPS = ((2,), (2, 11))
PROMPT = [5, 17, 40, 9]
LIMIT = 10
# (seed, weight scale, alpha): alpha shapes the stop ids' lm_head rows (alpha / |h|^2 * h, h = the prompt's last hidden state,
# is added: the stop ids' first-step logits rise by alpha).  Chosen on the CPU with transformers alone so that, over the grid,
# hypotheses finish before the step limit (alpha > 0), searches stop with beams still running, searches never meet a stop id
# (alpha = 0), and no step of any case has two neighbouring candidates (the K kept and the first one dropped) closer than 1e-4.
MODELS = ((0, 3.0, 0.0), (0, 3.0, 3.0), (0, 3.0, 6.0))


def _model(seed, scale, alpha, stops):
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(seed)
    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                      vocab_size=97, max_position_embeddings=64, pad_token_id=0, bos_token_id=1, eos_token_id=2)
    m = LlamaForCausalLM(cfg).eval().float()
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(scale)
        if alpha:
            h = m.model(torch.tensor([PROMPT])).last_hidden_state[0, -1]
            for s in stops:
                m.lm_head.weight[s] += alpha / float(h @ h) * h
    return m


def run_case(seed, scale, alpha, n, lp, es, stops):
    """(sequences equal, largest score difference, beam_ref's result) of one case"""
    stops = list(stops)
    m = _model(seed, scale, alpha, stops)
    prompt = torch.tensor([PROMPT])
    with torch.no_grad():
        out = m.generate(prompt, num_beams=n, do_sample=False, eos_token_id=stops, length_penalty=lp, early_stopping=es,
                         num_return_sequences=n, output_scores=True, return_dict_in_generate=True, max_new_tokens=LIMIT)

    def logits_fn(seqs, parents):
        with torch.no_grad():
            return m(torch.tensor([PROMPT + s for s in seqs])).logits[:, -1, :].float()

    r = beam_ref.search(logits_fn, n, stops, LIMIT, lp, es, dtype=torch.float32)
    hf = [row[len(PROMPT):].tolist() for row in out.sequences]
    ok = True
    if n == 1:
        # transformers runs num_beams = 1 as plain greedy search, which ends at the first stop id; a one-beam search goes on
        # with the best unfinished candidate.  They coincide wherever greedy meets no stop id, and there they must be equal.
        greedy = hf[0]
        if not any(t in stops for t in greedy):
            ok = greedy == r["sequences"][0]
        return ok, 0.0, r
    fill = stops[0]             # (transformers pads a shorter hypothesis with `pad_token_id or eos_token_id[0]`)
    for i in range(n):
        L = len(r["sequences"][i])
        ok = ok and r["finished"][i] and hf[i][:L] == r["sequences"][i] and all(t == fill for t in hf[i][L:])
    ds = max(abs(a - b) for a, b in zip(out.sequences_scores.tolist(), r["scores"]))
    return ok, ds, r


@functools.lru_cache(maxsize=None)
def _case(seed, scale, alpha, n, lp, es, stops):
    return run_case(seed, scale, alpha, n, lp, es, stops)


@pytest.mark.parametrize("stops", STOPS, ids=lambda s: "stops%d" % len(s))
@pytest.mark.parametrize("lp,es", SETTINGS, ids=lambda v: str(v))
@pytest.mark.parametrize("n", BEAMS)
@pytest.mark.parametrize("seed,scale,alpha", MODELS, ids=lambda v: str(v))
def test_beam_ref_equals_transformers(seed, scale, alpha, n, lp, es, stops):
    ok, ds, r = _case(seed, scale, alpha, n, lp, es, stops)
    assert ok, (r["sequences"], r["scores"])
    # sequences_scores to fp32 rounding: the two log-softmax routines may round each step's term differently (a few ulp at the
    # magnitude of the running sum S, which bounds every term and partial sum), LIMIT terms, one more rounding for the division
    S = max(abs(s) * len(q) ** lp for s, q in zip(r["scores"], r["sequences"]))
    assert ds <= 4 * LIMIT * 2.0 ** -23 * max(1.0, S), (ds, S)
    gap = min(beam_ref.min_gap(c) for c in r["steps"])
    assert gap >= 1e-4, gap


def test_beam_ref_grid_covers_the_paths():
    """the conditions on the chosen models, over the grid above (its cases are computed once)"""
    multi = []
    for (seed, scale, alpha), n, (lp, es), stops in itertools.product(MODELS, BEAMS[1:], SETTINGS, STOPS):
        r = _case(seed, scale, alpha, n, lp, es, stops)[2]
        multi.append((len(r["steps"]), [len(s) for s in r["sequences"]], [s[-1] in stops for s in r["sequences"]]))
    assert any(any(l < LIMIT for l in lens) for _, lens, _ in multi)            # a hypothesis finished before the step limit
    assert any(steps < LIMIT for steps, _, _ in multi)                           # a search stopped with beams still running
    assert any(not any(st) for _, _, st in multi)                                # a search never met a stop id


def test_beam_ref_step_tie_rule_and_masslesss_entries():
    rows = torch.zeros(3, 5)
    rows[1, 2] = float("nan")
    rows[2] = float("-inf")
    rows[2, 4] = 1.0
    c = beam_ref.step(rows, [0.0, 0.0, None], 6)
    # rows 0 and 1: uniform over 5 and over 4 entries; row 1 (fewer entries, more mass each) first, ties by ascending token
    assert [(b, t) for _, b, t in c] == [(1, 0), (1, 1), (1, 3), (1, 4), (0, 0), (0, 1)]
    assert c[0][0] == pytest.approx(-math.log(4)) and c[4][0] == pytest.approx(-math.log(5))
    c = beam_ref.step(rows, [None, None, -1.5], 4)
    assert c[0] == (-1.5, 2, 4) and c[1:] == [(float("-inf"), -1, -1)] * 3


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_beam_search():
    import ctypes as C
    from seedstory import _lib
    with open(os.path.join(ROOT, "include", "seedstory_hip.h")) as f:
        header = f.read()
    assert "#define SS_ABI_VERSION 1" in header
    for name in ("ss_beam_step", "ss_llama_beam_bytes", "ss_llama_beam_search", "ss_llama_beam_seq_offset", "ss_llama_beam_permute"):
        assert name + "(" in header and name in _lib.PROTOTYPES
    assert "typedef struct ss_beam_params" in header and "typedef struct ss_beam_state" in header
    lib = _lib.lib()
    assert lib.ss_abi_version() == 1
    # refused without a handle / with NULL buffers, before anything touches a device
    bp = _lib.BeamParams(2, 1.0, 0)
    assert lib.ss_llama_beam_search(None, C.byref(bp), None, 4, 1, None) == -1 and b"llama_beam_search" in lib.ss_last_error()
    assert lib.ss_llama_beam_permute(None, None, None, 2, 0, 0, None) == -1 and b"llama_beam_permute" in lib.ss_last_error()
    assert lib.ss_beam_step(None, 1, 10, 10, None, 0, None, None, None, None, 0, None) == -1 and b"beam_step" in lib.ss_last_error()
    # the workspace: head + row lists + 4 sequence buffers of n * max_new ids; 0 for a beam count the engine cannot take
    cfg = _lib.LlamaConfig(64, 2, 2, 128, 100, 64, 1e-5, 0, 64, 16, 0, 2, 4)
    off = lib.ss_llama_beam_seq_offset()
    assert off >= C.sizeof(_lib.BeamState) + 2 * 8 * 24 * 4 and off % 16 == 0
    assert lib.ss_llama_beam_bytes(C.byref(cfg), 4) == off + 4 * 4 * 16 * 4
    assert lib.ss_llama_beam_bytes(C.byref(cfg), 0) == 0 and lib.ss_llama_beam_bytes(C.byref(cfg), 9) == 0
    assert lib.ss_llama_beam_bytes(None, 2) == 0
    # the Python mirror of ss_beam_state: 16 words of scalars + 7 arrays of SS_BEAM_MAX words
    assert C.sizeof(_lib.BeamState) == 4 * (16 + 7 * _lib.BEAM_MAX) and "#define SS_BEAM_MAX 8" in header


# ---- LlamaForCausalLM.generate on the stand-in engine ---------------------------------------------------------------------------------
def _beam_llm(monkeypatch, winner, others=(), fail=None):
    """the stand-in engine of test_fork_cpu.py with a ``beam_search`` that answers ``winner`` (and ``others``), every call of
    interest recorded with its arguments in ``eng.log``"""
    from test_fork_cpu import IMG, _llm_and_engine
    m, eng, kw, touched = _llm_and_engine(monkeypatch)
    eng.log = []

    def beam_search(n_steps, last_prompt_id, num_beams, length_penalty=1.0, early_stopping=False):
        eng.log.append(("beam_search", n_steps, last_prompt_id, num_beams, length_penalty, early_stopping, eng.cur, eng.stop2,
                        len(eng.fed[0])))
        if fail is not None:
            raise fail
        for b in range(num_beams):                      # the slots are left with the running hypotheses' caches
            eng.fed[b] = eng.fed[0][:len(eng.fed[0])] + [900 + b] * 3
        seqs = [list(winner)] + [list(o) for o in others]
        seqs += [[]] * (num_beams - len(seqs))
        return {"sequences": seqs, "scores": torch.tensor([-0.5 - i for i in range(num_beams)]),
                "finished": torch.tensor([bool(s) for s in seqs])}

    eng.beam_search = beam_search
    for name in ("prefill", "generate", "set_lengths"):
        def wrap(*a, _f=getattr(eng, name), _n=name, **k):
            eng.log.append((_n,) + tuple(x.shape[0] if isinstance(x, torch.Tensor) else x for x in a))
            return _f(*a, **k)
        setattr(eng, name, wrap)
    return m, eng, kw, touched, IMG


def test_switch_off_nothing_new_is_called(monkeypatch):
    m, eng, kw, _, _ = _beam_llm(monkeypatch, [7, 8])
    assert m.beam_search is False
    a = m.generate(max_new_tokens=12, **kw)
    log_a, calls_a = list(eng.log), list(eng.calls)
    eng.log.clear()
    eng.calls.clear()
    b = m.generate(max_new_tokens=12, num_beams=4, length_penalty=2.0, early_stopping=True, **kw)
    assert a.sequences.tolist() == b.sequences.tolist() and b.beams is None and b.sequences_scores is None
    assert eng.log == log_a and eng.calls == calls_a and "beam_search" not in [c[0] for c in eng.log]     # call for call
    with pytest.raises(NotImplementedError):
        m.generate(max_new_tokens=12, num_beams=4, do_sample=True, **kw)


def test_switch_on_call_order_and_output(monkeypatch):
    win = [7, 8, 9]
    m, eng, kw, _, IMG = _beam_llm(monkeypatch, win, others=[[7, 5]])
    m.beam_search = True
    S = kw["input_ids"].shape[1]
    out = m.generate(max_new_tokens=12, num_beams=3, length_penalty=0.5, early_stopping="never", **kw)
    names = [c[0] for c in eng.log]
    assert names[:5] == ["prefill", "beam_search", "set_lengths", "prefill", "generate"], names
    # the search: the whole budget, from the prompt's last id, on slot 0, stopping at <img>, behind the S prompt rows
    assert eng.log[1] == ("beam_search", 12, 42, 3, 0.5, "never", 0, IMG[0], S)
    assert eng.stop2 == -1
    # the winner made real: back to the prompt end, t_1 .. t_{m-1} as one prefill, t_m forced with the remaining budget
    assert eng.log[2] == ("set_lengths", S, S) and eng.log[3] == ("prefill", 2)
    assert eng.log[4][:4] == ("generate", 12 - 2, 8, [9])
    gen = out.sequences[0, S:].tolist()
    assert gen[:3] == win and len(gen) == 12 and out.sequences[0, :S].tolist() == kw["input_ids"][0].tolist()
    assert eng.fed[0][:S + 2] == kw["input_ids"][0].tolist() + win[:2]                   # slot 0 holds the winner, not a beam
    assert len(out.hidden_states) == 1 + len(gen) - 1
    assert out.sequences_scores.tolist() == [-0.5]
    assert [b["sequence"] for b in out.beams] == [win, [7, 5], []] and [b["finished"] for b in out.beams] == [True, True, False]
    assert out.candidates is None


def test_winner_ending_in_img_runs_the_block(monkeypatch):
    m, eng, kw, _, IMG = _beam_llm(monkeypatch, [7, 3000])
    assert IMG[0] == 3000
    m.beam_search = True
    m.use_kv_cache_head = True
    S = kw["input_ids"].shape[1]
    out = m.generate(max_new_tokens=80, num_beams=2, **kw)
    gen = out.sequences[0, S:].tolist()
    assert gen[:2] == [7, IMG[0]] and gen[2:2 + 65] == IMG[1:]                           # the forced block behind the winner
    assert m.kv_cache_head == S + len(gen) - 1
    # a second generate from the returned cache goes on from the winner
    eng.log.clear()
    m.beam_search = False
    nxt = torch.cat([out.sequences, torch.tensor([[11]])], dim=1)
    m.generate(input_ids=nxt, inputs_embeds=nxt.float().unsqueeze(-1), logits_processor=kw["logits_processor"],
               past_key_values=m.past_key_values, max_new_tokens=4)
    assert eng.log[0][0] == "prefill" and eng.fed[0][:S + 2] == kw["input_ids"][0].tolist() + [7, IMG[0]]


def test_refusals_come_before_the_engine(monkeypatch):
    m, eng, kw, touched, _ = _beam_llm(monkeypatch, [7, 8])
    m.beam_search = True
    with pytest.raises(ValueError, match="n_seq"):
        m.generate(max_new_tokens=12, num_beams=5, **kw)                                 # the stand-in has 4 slots
    with pytest.raises(ValueError, match="forced_tokens"):
        m.generate(max_new_tokens=12, num_beams=2, forced_tokens=[5], **kw)
    with pytest.raises(ValueError):
        m.generate(max_new_tokens=12, num_beams=2, num_return_sequences=2, **kw)
    with pytest.raises(ValueError, match="early_stopping"):
        m.generate(max_new_tokens=12, num_beams=2, early_stopping="always", **kw)
    with pytest.raises(NotImplementedError):
        m.generate(max_new_tokens=12, num_beams=2, output_attentions=True, **kw)
    with pytest.raises(NotImplementedError):
        m.generate(max_new_tokens=12, num_beams=2, output_logprobs=True, **kw)
    m.kv_cache = "fp8"
    with pytest.raises(NotImplementedError, match="fp8"):
        m.generate(max_new_tokens=12, num_beams=2, **kw)
    m.kv_cache = None
    with pytest.raises(NotImplementedError):
        m.generate(max_new_tokens=12, num_beams=2, do_sample=True, **kw)
    assert touched == [] and eng.log == [] and eng.calls == []


def test_state_is_restored_when_the_search_raises(monkeypatch):
    from seedstory import _lib
    m, eng, kw, _, _ = _beam_llm(monkeypatch, [7, 8], fail=_lib.SSError("boom"))
    m.beam_search = True
    with pytest.raises(_lib.SSError, match="boom"):
        m.generate(max_new_tokens=12, num_beams=2, no_repeat_ngram_size=2, **kw)
    assert eng.stop2 == -1 and eng.rules is None and eng._rules_slots == set()
    assert [c[0] for c in eng.calls if c[0] in ("rules", "rules_off")] == ["rules", "rules_off"]
    # rules reach every beam: set for all slots, the prompt handed over as slot 0's history before the search
    assert ("rules", None) in eng.calls and ("history", 0, False) in eng.calls
