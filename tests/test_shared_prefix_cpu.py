"""The shared-prefix case table (tests/shared_prefix_cases.py) without a GPU: every case's defect floor - how far the mildest modelled
fault of the redirect moves the oracle's logits - reaches 2e-3, so the GPU tests' differential bound floor / 4 separates a correct
engine from a boundary that is off by one; the table holds the prefixes at the tile edges of both compute dtypes; the inputs are what
the defect models assume; and the decode cases' row counts really plan the attention forms they are listed for."""
import ctypes as C

import numpy as np
import pytest
import torch

import shared_prefix_cases as sp


@pytest.mark.parametrize("name", [c.name for c in sp.CASES])
def test_defect_floor_reaches_the_minimum(name):
    c = sp.BY_NAME[name]
    ref = sp.reference(name)
    assert c.context <= 152, c.context
    expect = {("M2", s) for s in range(1, c.slots)} | {("M1", s) for s in range(c.N, c.slots)} | \
             {("M3", s) for s in range(c.slots) if s % c.N}
    assert set(ref["models"]) == expect
    assert sp.defect_floor(c) == min(ref["models"].values())
    assert sp.defect_floor(c) >= sp.FLOOR_MIN, (c.context, ref["models"])


def test_prefixes_sit_on_the_tile_edges_of_both_dtypes():
    for dtype, kw in sp.KW.items():
        have = {c.P for c in sp.CASES if c.dtype == dtype}
        assert {kw - 1, kw, kw + 1, 2 * kw, 63, 64, 65} <= have, (dtype, sorted(have))
    assert {c.preset for c in sp.CASES} == {"tiny", "tiny128", "tiny_h16"}
    fam = {c.family for c in sp.CASES}
    assert fam == {"prefill", "prefill64", "multipass", "decode", "refill", "retire", "best_of"}, fam
    for c in sp.CASES:
        if c.family == "refill":          # the boundary lies behind the first batch of 4 * 8 * PPW positions (head_dim 128: PPW = 4 in bf16, 2 in fp32)
            assert c.preset == "tiny128" and c.P - 1 >= (128 if c.dtype == "bf16" else 64)
        if c.family == "prefill64":       # every prompt has at least one 64-row block after the skip, one of them a ragged last block
            rows = [n + c.T + 1 for n in c.lens[1:]]
            assert min(rows) >= 64 and any(r % 64 for r in rows) and any(r % 64 == 0 for r in rows), rows
        if c.family == "retire":          # text 0 is through several steps before the last compared one
            assert c.ends[0] + 4 + 3 <= c.steps <= min(c.ends[1:])


@pytest.mark.parametrize("name", ["pf-tiny-fp32-P17", "bestof-tiny_h16-bf16-P64", "retire-tiny128-bf16-P33-sh1"])
def test_inputs_share_exactly_the_prefix_and_the_stale_call_shares_nothing(name):
    c = sp.BY_NAME[name]
    a, _ = sp.model(c.preset)
    texts, stale, y, y_stale, forced = sp.inputs(name)
    assert len(set(c.lens)) == len(c.lens) or c.family in ("decode", "refill")
    assert len({int(t[c.P]) for t in texts}) == c.B                    # they differ AT index P
    for u, (t, st) in enumerate(zip(texts, stale)):
        assert t.numel() == c.P + c.lens[u] == st.numel()
        assert torch.equal(t[: c.P], texts[0][: c.P])
        assert not (t == st).any() and 0 <= int(st.min()) and int(st.max()) < a.text_vocab_size
    assert y.shape == y_stale.shape == (c.T, a.n_codebooks) and not torch.equal(y, y_stale)
    K = a.n_codebooks
    assert forced.shape[1:] == (c.slots, K)
    for s in range(c.slots):
        e = c.end(s)
        assert [int(forced[e + j, s, j]) for j in range(K)] == [a.eos] * K
        assert (forced[:e, s] < a.audio_vocab_size).all()


def test_prefix_oracle_without_substitution_is_the_oracle_and_records_the_prefill():
    from oracle.voicecraft_oracle import VoiceCraftOracle
    c = sp.BY_NAME["pf-tiny-fp32-P17"]
    a, sd = sp.model(c.preset)
    texts, stale, y, y_stale, forced = sp.inputs(c.name)
    x = texts[1]
    trace = []
    VoiceCraftOracle(a, sd).inference_tts(x.unsqueeze(0), torch.tensor([x.numel()]), y.unsqueeze(0), top_k=1, stop_repetition=3,
                                          trace=trace, forced=forced[:, 1], max_steps=c.steps)
    want = torch.stack([t["logits"][0] for t in trace]).numpy()
    orc = sp.PrefixOracle(a, sd)
    got, rec = orc.run(x, y, forced[:, 1], c.steps)
    assert np.array_equal(got, want) and np.array_equal(got, sp.reference(c.name)["clean"][1])
    S0 = x.numel() + c.T + 1
    assert sorted(rec) == list(range(a.num_decoder_layers))
    assert all(k.shape == v.shape == (1, a.nhead, S0, a.d_model // a.nhead) for k, v in rec.values())
    # a row substituted by itself changes nothing; by another text's row it does, and only from that position's reader on
    same, _ = orc.run(x, y, forced[:, 1], c.steps, subst=[(c.P, rec)])
    assert np.array_equal(same, want)
    other, _ = orc.run(x, y, forced[:, 1], c.steps, subst=[(c.P, sp.PrefixOracle(a, sd).run(texts[0], y, forced[:, 0], 1)[1])])
    assert sp.rel_l2(other, want).min() > 1e-3


def test_decode_cases_plan_the_forms_they_are_listed_for():
    """vc_debug_plan (the engine's own plan_pass, host only): rows -> (form, attention splits) of a decode step."""
    from voicecraft_amd import _lib
    from voicecraft_amd._lib import ModelCfg
    lib = _lib.load()
    seen = set()
    for c in sp.CASES:
        if not c.plan:
            continue
        a, _ = sp.model(c.preset)
        rows, form, nsplit = c.plan
        assert rows == c.slots
        av = a.audio_vocab_size
        cfg = ModelCfg(d_model=a.d_model, nhead=a.nhead, num_layers=a.num_decoder_layers, n_codebooks=a.n_codebooks, audio_vocab_size=av,
                       n_special=a.n_special, text_rows=a.text_vocab_size + 1, head_hidden=av // 2, empty_token=a.empty_token, eog=a.eog,
                       audio_pad_token=a.audio_pad_token, eos=a.eos, reduced_eog=1, encodec_sr=50, max_n_spans=3, max_seqs=max(rows, 2),
                       max_positions=256)
        out = (C.c_int32 * 16)()
        assert lib.vc_debug_plan(C.byref(cfg), _lib.VC_DTYPE_BF16 if c.dtype == "bf16" else _lib.VC_DTYPE_F32, rows, out) == 0
        assert (out[1], out[2]) == (form, nsplit), (c.name, list(out))
        if form == sp.FORM_WIDE:
            assert out[11] == 1 and dict(c.census)["wd"], c.name
        seen.add((c.dtype, form, nsplit))
    for dtype in ("bf16", "fp32"):
        assert {(dtype, sp.FORM_FR, n) for n in (8, 4, 2, 1)} | {(dtype, sp.FORM_WIDE, 1)} <= seen
