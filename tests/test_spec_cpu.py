"""Host side of prompt-lookup speculative decoding (no GPU): ``tests/spec_ref.py`` pinned against the installed transformers'
``PromptLookupCandidateGenerator``, the step / replay model's own invariants, the C ABI's new names, and the plumbing of
``LlamaEngine.set_speculation`` over a recording stand-in library."""
import ctypes as C
import os

import pytest
import torch

import spec_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- spec_ref.draft == transformers ------------------------------------------------------------------------------------------------
GRID = spec_ref.draft_grid()


def _hf(seq, g, k, stops):
    from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    gen = PromptLookupCandidateGenerator(eos_token_id=torch.tensor(stops) if stops else None, num_output_tokens=k,
                                         max_matching_ngram_size=g, max_length=10 ** 6)
    ids = torch.tensor([seq], dtype=torch.long)
    cand, _ = gen.get_candidates(ids)
    return cand[0, len(seq):].tolist()


def test_draft_equals_transformers_prompt_lookup():
    for seq, g, k, stops in GRID:
        assert spec_ref.draft(seq, g, k, stops) == _hf(seq, g, k, stops), (seq, g, k, stops)


def test_draft_grid_reaches_every_path():
    seen = set()
    for seq, g, k, stops in GRID:
        spec_ref.draft(seq, g, k, stops)
        seen |= set(spec_ref.draft.path.split("+"))
        seen.add(spec_ref.draft.path)
    for path in ("none", "match", "clipped", "stop", "fallback"):
        assert path in seen, (path, sorted(seen))
    # a stop id at the head of the continuation: no draft, and no shorter n-gram is tried (transformers breaks out there)
    assert spec_ref.draft([1, 2, 9, 3, 2, 5, 1, 2], 2, 3, (9,)) == [] == _hf([1, 2, 9, 3, 2, 5, 1, 2], 2, 3, (9,))


# ---- the step model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", (2, 3, 4, 8))
@pytest.mark.parametrize("n_tok", (1, 2, 7, 8, 9, 17))
def test_replay_all_accepted_emits_rows_per_step(rows, n_tok):
    ids = [10 + i for i in range(n_tok)]
    r = spec_ref.replay(ids, rows=rows, limit=n_tok, max_new=64, kv_room=64, pos_room=64, source="given", given=ids)
    assert r["ids"] == ids and r["emitted"] == n_tok
    # n tokens need n - 1 forwards (the last token of a call is never fed): ceil((n - 1) / rows) steps, every draft accepted
    assert r["steps"] == -(-(n_tok - 1) // rows)
    assert r["accepted"] == r["drafted"] == (n_tok - 1) - r["steps"]
    assert r["kv_advance"] == n_tok - 1
    assert all(len(t) == rows for t, _ in r["per_step"][:-1])


def test_replay_rejections_forced_stops_and_room():
    ids = [10 + i for i in range(12)]
    bad = list(ids)
    bad[3] = 99                         # draft for index 3 is wrong: the step that drafts it accepts only what lies before it
    r = spec_ref.replay(ids, rows=4, limit=12, max_new=64, kv_room=64, pos_room=64, source="given", given=bad)
    assert r["ids"] == ids and r["kv_advance"] == 11
    assert r["per_step"][0] == ([10, 11, 12, 99], 2) and r["per_step"][1][0] == [13, 14, 15, 16]
    assert r["accepted"] == r["drafted"] - 1
    # a stop id ends the call where greedy ends it; it is never drafted
    r = spec_ref.replay(ids[:6] + [2], rows=4, limit=12, max_new=64, kv_room=64, pos_room=64, source="given", given=ids[:6] + [2],
                        stops=(2,))
    assert r["ids"] == ids[:6] + [2] and r["kv_advance"] == 6 and all(2 not in t for t, _ in r["per_step"])
    # forced ids are certain drafts, whatever the source
    r = spec_ref.replay(ids, rows=4, limit=12, max_new=64, kv_room=64, pos_room=64, source="lookup", forced=ids[:5], hist=[1, 2, 3])
    assert r["per_step"][0] == (ids[:4], 3) and r["ids"] == ids
    # cache room: rows are clipped, never the tokens
    r = spec_ref.replay(ids, rows=8, limit=12, max_new=64, kv_room=11, pos_room=64, source="given", given=ids)
    assert r["ids"] == ids and r["kv_advance"] == 11
    # lookup: a repeating sequence is drafted from its own past
    loop = [5, 6, 7] * 6
    r = spec_ref.replay(loop[3:], rows=4, limit=15, max_new=64, kv_room=64, pos_room=64, source="lookup", hist=loop[:3], max_ngram=2)
    assert r["ids"] == loop[3:] and r["accepted"] == r["drafted"] > 0


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_speculation():
    from seedstory import _lib
    with open(os.path.join(ROOT, "include", "seedstory_hip.h")) as f:
        header = f.read()
    assert "#define SS_ABI_VERSION 1" in header
    for name in ("ss_llama_spec_bytes", "ss_llama_set_speculation", "ss_llama_spec_stats", "ss_attn_decode_spec", "ss_spec_draft"):
        assert name + "(" in header and name in _lib.PROTOTYPES
    assert "typedef struct ss_spec_params" in header and "#define SS_SPEC_MAX_ROWS 8" in header
    lib = _lib.lib()
    assert lib.ss_abi_version() == 1
    # refused on NULL arguments, before anything touches a device; each names itself
    n = C.c_size_t()
    out = (C.c_int64 * 4)()
    assert lib.ss_llama_spec_bytes(None, 4, C.byref(n)) == -1 and b"llama_spec_bytes" in lib.ss_last_error()
    assert lib.ss_llama_set_speculation(None, None, None) == -1 and b"llama_set_speculation" in lib.ss_last_error()
    assert lib.ss_llama_spec_stats(None, 0, out) == -1 and b"llama_spec_stats" in lib.ss_last_error()
    assert lib.ss_attn_decode_spec(*([None] * 10), 2, 2, 64, 16, 0, None) == -1 and b"attn_decode_spec" in lib.ss_last_error()
    assert lib.ss_spec_draft(None, 4, 2, 3, 0, None, None, None, None) == -1 and b"spec_draft" in lib.ss_last_error()
    # the workspace: grows with the rows, refused outside 2..8
    cfg = _lib.LlamaConfig(64, 2, 2, 128, 100, 64, 1e-5, 0, 64, 16, 0, 2, 1)
    sizes = []
    for rows in (2, 4, 8):
        assert lib.ss_llama_spec_bytes(C.byref(cfg), rows, C.byref(n)) == 0
        sizes.append(n.value)
        # R rows of x, xn, attn (hidden), qkv (3 hidden), hm (inter), logits (vocab) in bf16 + R attention partial slabs
        assert n.value >= rows * (2 * (6 * 64 + 128 + 100) + lib.ss_attn_decode_workspace_bytes(2, 32))
    assert sizes[0] < sizes[1] < sizes[2]
    for rows in (0, 1, 9):
        assert lib.ss_llama_spec_bytes(C.byref(cfg), rows, C.byref(n)) == -1 and b"rows" in lib.ss_last_error()
    assert C.sizeof(_lib.SpecParams) == 24


# ---- LlamaEngine plumbing over a recording library ------------------------------------------------------------------------------------
class _FakeLib:
    """records every call made through it; the ``ss_llama_*`` calls answer 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name == "ss_llama_spec_bytes":
                args[2]._obj.value = 4096
            if name == "ss_llama_generate":
                args[5]._obj.value = 3
            if name == "ss_llama_spec_stats":
                for i in range(4):
                    args[2][i] = 10 + i
            return 0
        return call


@pytest.fixture
def fake_engine(monkeypatch):
    from seedstory import _lib, llama
    fake = _FakeLib()
    monkeypatch.setattr(llama, "lib", lambda: fake)
    monkeypatch.setattr(llama, "check", lambda rc, what="": None)
    monkeypatch.setattr(llama.ops, "stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"synchronize": lambda self: None})())
    eng = llama.LlamaEngine.__new__(llama.LlamaEngine)
    eng.device = torch.device("cpu")
    eng._h = C.c_void_p(1)
    eng._cfg = _lib.LlamaConfig(64, 2, 2, 128, 100, 64, 1e-5, 0, 64, 16, 0, 2, 1)
    eng._spec, eng.speculate, eng._rules_slots, eng._cur, eng.n_seq = None, 0, set(), 0, 1
    yield eng, fake
    eng._h = None


def test_engine_generate_calls_nothing_new_with_speculation_off(fake_engine):
    eng, fake = fake_engine
    assert eng.generate(5, 7, forced=[1, 2]) == 3
    assert [c[0] for c in fake.calls] == ["ss_llama_generate"]
    args = fake.calls[0][1]
    assert args[1] == 5 and args[2] == 7 and list(args[3])[:2] == [1, 2] and args[4] == 2


def test_engine_set_speculation_call_order_and_pass_through(fake_engine):
    from seedstory import _lib
    eng, fake = fake_engine
    eng.set_speculation(4, max_ngram=3)
    assert [c[0] for c in fake.calls] == ["ss_llama_spec_bytes", "ss_llama_set_speculation"]
    assert fake.calls[0][1][1] == 4
    sp = fake.calls[1][1][1]._obj
    assert (sp.rows, sp.max_ngram, sp.source, sp.given_len, sp.given_ids) == (4, 3, _lib.SPEC_LOOKUP, 0, None)
    assert fake.calls[1][1][2] == eng._spec[0].data_ptr() and eng._spec[0].numel() == 4096 and eng.speculate == 4
    # generate is the call it always was: the engine holds the option
    assert eng.generate(5, 7) == 3 and fake.calls[2][0] == "ss_llama_generate"
    assert eng.spec_stats() == {"steps": 10, "drafted": 11, "accepted": 12, "emitted": 13}
    # given drafts travel as an int32 array of their own
    eng.set_speculation(2, draft_ids=[4, 5, 6])
    sp = fake.calls[-1][1][1]._obj
    assert (sp.rows, sp.source, sp.given_len) == (2, _lib.SPEC_GIVEN, 3) and sp.given_ids == eng._spec[1].data_ptr()
    assert eng._spec[1].dtype == torch.int32 and eng._spec[1].tolist() == [4, 5, 6]
    # image-block tokens join the history while the option is on (they feed the drafts)
    n = len(fake.calls)
    eng._history_append(0, [8, 9])
    assert [c[0] for c in fake.calls[n:]] == ["ss_llama_set_history"] and fake.calls[-1][1][4] == 1
    eng.clear_speculation()
    assert fake.calls[-1][0] == "ss_llama_set_speculation" and fake.calls[-1][1][1] is None and fake.calls[-1][1][2] is None
    assert eng._spec is None and eng.speculate == 0
    n = len(fake.calls)
    eng._history_append(0, [8, 9])
    assert len(fake.calls) == n


@pytest.mark.parametrize("kw", (dict(rows=1), dict(rows=9), dict(rows=4, max_ngram=0), dict(rows=4, max_ngram=9)))
def test_engine_set_speculation_refuses_before_any_call(fake_engine, kw):
    eng, fake = fake_engine
    with pytest.raises(ValueError):
        eng.set_speculation(**kw)
    assert fake.calls == []


def test_knob_is_declared_with_default_off():
    from seedstory import _lib
    assert _lib.get_tuning("llama_spec_rows", -5) == 0


# ---- LlamaForCausalLM.generate on the stand-in engine of test_fork_cpu.py -------------------------------------------------------------
def _spec_llm(monkeypatch):
    from test_fork_cpu import _llm_and_engine
    m, eng, kw, touched = _llm_and_engine(monkeypatch)

    def set_speculation(rows, max_ngram=2, draft_ids=None):
        eng.calls.append(("speculation", rows, max_ngram, draft_ids))

    eng.set_speculation = set_speculation
    eng.clear_speculation = lambda: eng.calls.append(("speculation_off",))
    return m, eng, kw, touched


def _names(eng):
    return [c[0] for c in eng.calls]


def test_generate_switch_off_calls_nothing_new(monkeypatch):
    m, eng, kw, _ = _spec_llm(monkeypatch)
    assert type(m).speculative == 0
    a = m.generate(max_new_tokens=12, **kw)
    calls = list(eng.calls)
    eng.calls.clear()
    b = m.generate(max_new_tokens=12, prompt_lookup_num_tokens=3, max_matching_ngram_size=2, **kw)      # inert while the switch is 0
    assert eng.calls == calls and "speculation" not in _names(eng) and "history" not in _names(eng)
    assert torch.equal(a.sequences, b.sequences)


def test_generate_switch_on_order_and_pass_through(monkeypatch):
    m, eng, kw, _ = _spec_llm(monkeypatch)
    ref = m.generate(max_new_tokens=12, **kw)
    eng.calls.clear()
    m.speculative = 1
    out = m.generate(max_new_tokens=12, prompt_lookup_num_tokens=3, max_matching_ngram_size=4, **kw)
    names = _names(eng)
    assert names[:2] == ["speculation", "history"] and names[-1] == "speculation_off" and "generate" in names[2:-1]
    assert eng.calls[0] == ("speculation", 4, 4, None)                          # k drafts = k + 1 rows
    assert eng.calls[1] == ("history", 0, False) and eng.hist[0] == kw["input_ids"][0].tolist()
    assert torch.equal(out.sequences, ref.sequences)
    # rows are capped at 8, the n-gram default is Hugging Face's 2; without the keyword nothing is set
    eng.calls.clear()
    m.generate(max_new_tokens=12, prompt_lookup_num_tokens=10, **kw)
    assert eng.calls[0] == ("speculation", 8, 2, None)
    eng.calls.clear()
    m.generate(max_new_tokens=12, **kw)
    assert "speculation" not in _names(eng)
    # batch calls are what they were: the option is not set for best-of-n
    eng.calls.clear()
    m.generate(max_new_tokens=12, prompt_lookup_num_tokens=3, do_sample=True, seed=1, num_return_sequences=2, **kw)
    assert "speculation" not in _names(eng) and "generate_batch" in _names(eng)
    # switched off again when the call raises
    eng.calls.clear()
    eng.generate = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("boom"))
    with pytest.raises(RuntimeError):
        m.generate(max_new_tokens=12, prompt_lookup_num_tokens=3, **kw)
    assert _names(eng)[-1] == "speculation_off"


@pytest.mark.parametrize("kw2,exc", [
    (dict(do_sample=True), NotImplementedError), (dict(repetition_penalty=1.3), NotImplementedError),
    (dict(no_repeat_ngram_size=2), NotImplementedError), (dict(min_new_tokens=4), NotImplementedError),
    (dict(output_logprobs=True), NotImplementedError), (dict(output_attentions=True), NotImplementedError),
    (dict(max_matching_ngram_size=0), ValueError), (dict(max_matching_ngram_size=9), ValueError)])
def test_generate_refusals_before_the_engine_is_touched(monkeypatch, kw2, exc):
    m, eng, kw, touched = _spec_llm(monkeypatch)
    m.speculative = 1
    with pytest.raises(exc):
        m.generate(max_new_tokens=12, prompt_lookup_num_tokens=3, **kw2, **kw)
    assert eng.calls == [] and touched == []


def test_generate_refuses_fp8_kv_cache(monkeypatch):
    m, eng, kw, touched = _spec_llm(monkeypatch)
    m.speculative, m.kv_cache = 1, "fp8"
    with pytest.raises(NotImplementedError, match="kv_cache"):
        m.generate(max_new_tokens=12, prompt_lookup_num_tokens=3, **kw)
    assert eng.calls == [] and touched == []
