"""-m gpu: option `w8` - on an engine created with `w8=`, one-row steps stream the FFN down-projection (bit 1) and the QKV projection
(bit 4) as one E4M3 byte per value and one shift byte per 512-value fragment (vc_gemm_w8.hip, vc_w8.h).  The bytes decode to the same
bf16 operands, the kernels keep the prologue, epilogue and summation order of their bf16 twins: teacher-forced head logits are
BIT-identical to option off (`w8 = 0` runs the `w13` path, `w13 = 0` the bf16 images), under the captured graph and eager, at every
width at which the kernels take another form (the shapes of tests/test_gpu_w13.py).  What the quantisation itself costs is not tested
here beyond the project's bf16 bar against the oracle ON the quantised checkpoint: that is a CPU measurement."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_STEPS = 12
SHAPES = {"tiny128": None, "tiny_h16": None, "giga330M": 2, "giga830M": 1}      # preset -> decoder layers (None: the preset's own)
OFF_GRID = (1.0 + 2.0 ** -7) * 2.0 ** -6                                        # eight significant bits: on no E4M3 grid


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


@functools.lru_cache(maxsize=None)
def _model(preset):
    """(args, plain synthetic state dict, the same on the w8 grid, prompt, forced tokens): computed once, never modified."""
    from voicecraft_amd import quant, synth
    kw = {} if SHAPES.get(preset) is None else {"num_decoder_layers": SHAPES[preset]}
    a = synth.make_args(preset, **kw)
    sd = synth.make_state_dict(a, seed=0, fast=True)
    x, xl, y = synth.random_prompt(a, 6, 20, seed=3)
    K = a.n_codebooks
    toks = np.random.RandomState(17).randint(0, a.audio_vocab_size, size=(N_STEPS, K)).astype(np.int64)
    for j in range(K):                      # the staggered end of the span (voicecraft.py:1057-1066): the call ends with its forced steps
        toks[N_STEPS - K + j, :j] = a.empty_token
        toks[N_STEPS - K + j, j] = a.eos
    return a, sd, quant.quantize_state_dict_w8(a, sd), (x, xl, y), toks


def _engine(a, sd, w8, use_graph=True, dtype="bf16", cls=None):
    from voicecraft_amd.engine import VoiceCraftEngine
    kw = {} if w8 == "none" else {"w8": w8}
    return (cls or VoiceCraftEngine)(a, sd, device="cuda:0", dtype=dtype, max_seqs=1, max_positions=256, use_graph=use_graph, **kw)


def _logits(eng, prompt, toks):
    x, xl, y = prompt
    _, _, lg = eng.inference_tts(x.cuda(), xl.cuda(), y.cuda(), top_k=1, stop_repetition=3, _forced=toks, _logit_steps=len(toks))
    return lg.cpu().numpy()


def _applicable(d):
    return (1 if d >= 512 else 0) | (4 if d >= 1024 else 0)


def _same_dict(sd1, sd2):
    return set(sd1) == set(sd2) and all(torch.equal(sd1[k], sd2[k]) for k in sd1 if torch.is_tensor(sd1[k]))


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("preset", list(SHAPES))
def test_w8_logits_bit_identical_and_census(preset, use_graph):
    a, sd, sdq, prompt, toks = _model(preset)
    eng = _engine(a, sd, "quantize", use_graph)
    assert _same_dict(eng.w8_state_dict, sdq) and not _same_dict(eng.w8_state_dict, sd)
    assert eng.options().endswith("|w13=5|w8=5")
    app = _applicable(a.d_model)
    for layer in eng.w8_stats():
        for bit, m in zip((1, 4), eng.W8_MATRICES):
            assert layer[m] == {"state": "packed" if app & bit else "not_applicable", "refused_fragments": 0}, (m, layer)
    assert eng.w13_stats() == eng.w8_stats()            # the quantised matrices have their 13-bit planes as well
    eng.set_option("w8", 0)
    eng.set_option("w13", 0)
    c0 = eng.launch_counts()
    want = _logits(eng, prompt, toks)
    c_off = _delta(eng.launch_counts(), c0)
    assert c_off["w8"] == 0 and c_off["w13"] == 0 and c_off["row_gemm_fr1"] > 0, c_off
    assert np.isfinite(want[np.abs(want) < 1e3]).all() and np.abs(want).max() > 0
    for w13, v in ((5, 0), (5, 5), (5, 1), (5, 4), (0, 5), (0, 1), (0, 4)):
        eng.set_option("w13", w13)
        eng.set_option("w8", v)
        assert eng.options().endswith(f"|w13={w13}|w8={v}")
        c0 = eng.launch_counts()
        got = _logits(eng, prompt, toks)
        c = _delta(eng.launch_counts(), c0)
        assert np.array_equal(got, want), (w13, v, float(np.abs(got - want).max()))
        # one paired QKV projection and one FFN down-projection per layer and step, each counted in its bf16 twin's slot and once more in
        # `w8` or `w13`: the w8 bit wins, the w13 slot counts the rest (tests/test_gpu_w13.py on eager / captured totals)
        assert c["row_gemm_fr1"] > 0 and c["row_gemm_fr1"] % 2 == 0 and c["rows_gemm"] > 0, (w13, v, c)
        per = c["row_gemm_fr1"] // 2
        assert c["w8"] == per * bin(v & app).count("1"), (w13, v, c)
        assert c["w13"] == per * bin(w13 & app & ~v).count("1"), (w13, v, c)


@pytest.mark.parametrize("preset", ["tiny128", "tiny_h16"])
def test_w8_engine_and_plain_bf16_engine_against_the_oracle_on_the_quantised_checkpoint(preset):
    """The quantised state dict is an ordinary checkpoint: the oracle runs on it unchanged, and both the w8 engine and a bf16 engine
    created without w8 meet the project's bf16 bar (per-step relative L2 <= 2e-2) against it - with identical logits."""
    from oracle.voicecraft_oracle import VoiceCraftOracle
    from test_gpu_model import rel_l2
    a, sd, sdq, prompt, toks = _model(preset)
    eng = _engine(a, sd, "quantize")
    torch.set_num_threads(min(4, torch.get_num_threads()))
    orc = VoiceCraftOracle(a, eng.w8_state_dict)
    want = orc.tts_logits_for_trajectory(prompt[0], prompt[2], toks, steps=list(range(len(toks)))).numpy()
    c0 = eng.launch_counts()
    got = _logits(eng, prompt, toks)
    assert _delta(eng.launch_counts(), c0)["w8"] > 0
    plain = _logits(_engine(a, eng.w8_state_dict, "none"), prompt, toks)
    for tag, lg in (("w8", got), ("bf16", plain)):
        rel = float(rel_l2(lg.reshape(want.shape), want).max())
        print(f"{preset} {tag} engine against the oracle on the quantised checkpoint: worst rel L2 {rel:.2e}")
        assert rel <= 2e-2, (tag, rel)
    assert np.array_equal(got, plain)


def test_w8_every_code_at_three_shifts_packs_and_decodes():
    """Layer 0's FFN down-projection holds all 254 non-NaN codes (+-0 among them) in each of three corner fragments, at three shifts."""
    a, sd, sdq, prompt, toks = _model("tiny128")
    sdq = {k: v.clone() for k, v in sdq.items()}
    w = sdq["decoder.layers.0.linear2.weight"]
    codes = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)
    vals = codes.view(torch.float8_e4m3fn).float()
    assert vals.numel() == 254 and bool(torch.isfinite(vals).all()) and float(vals.abs().max()) == 448.0
    frag = torch.cat([vals, vals, torch.tensor([0.0, -0.0, 448.0, -448.0])]).reshape(8, 64)
    for (r, c), s in (((0, 0), -16), ((8, 0), -13), ((0, 64), -10)):
        w[r:r + 8, c:c + 64] = frag * 2.0 ** s
    eng = _engine(a, sdq, "as_is")
    assert all(layer["ffn_down"] == {"state": "packed", "refused_fragments": 0} for layer in eng.w8_stats()), eng.w8_stats()
    eng.set_option("w8", 0)
    want = _logits(eng, prompt, toks)
    eng.set_option("w8", 5)
    c0 = eng.launch_counts()
    got = _logits(eng, prompt, toks)
    assert _delta(eng.launch_counts(), c0)["w8"] > 0
    assert np.isfinite(want[np.abs(want) < 1e3]).all() and np.array_equal(got, want), float(np.abs(got - want).max())


@pytest.mark.parametrize("preset", ["tiny128", "giga330M"])
def test_w8_as_is_on_plain_weights_refuses_every_matrix(preset):
    """Plain synthetic weights are on no 8-bit grid: every requested matrix comes back refused, and the engine launches and computes
    what an engine created without w8 does (captured graphs: each launch is counted once, at capture)."""
    a, sd, sdq, prompt, toks = _model(preset)
    app = _applicable(a.d_model)
    out = {}
    for w8 in ("as_is", "none"):
        eng = _engine(a, sd, w8)
        if w8 == "as_is":
            for layer in eng.w8_stats():
                for bit, m in zip((1, 4), eng.W8_MATRICES):
                    assert layer[m]["state"] == ("refused" if app & bit else "not_applicable"), (m, layer)
                    assert (layer[m]["refused_fragments"] > 0) == bool(app & bit), (m, layer)
            assert eng.options().endswith("|w13=5|w8=5")
        c0 = eng.launch_counts()
        lg = _logits(eng, prompt, toks)
        out[w8] = (lg, _delta(eng.launch_counts(), c0))
        del eng
    assert out["as_is"][1] == out["none"][1] and out["none"][1]["w8"] == 0 and out["none"][1]["w13"] > 0, out
    assert np.array_equal(out["as_is"][0], out["none"][0])


@pytest.mark.parametrize("preset", ["tiny128", "giga330M"])
def test_w8_one_off_grid_value_refuses_exactly_its_matrix(preset):
    a, sd, sdq, prompt, toks = _model(preset)
    sdq = {k: v.clone() for k, v in sdq.items()}
    sdq["decoder.layers.1.linear2.weight"][40, 200] = OFF_GRID
    eng = _engine(a, sdq, "as_is", use_graph=False)
    L = a.num_decoder_layers
    qkv = bool(_applicable(a.d_model) & 4)
    st = eng.w8_stats()
    for l in range(L):
        assert st[l]["qkv"] == {"state": "packed" if qkv else "not_applicable", "refused_fragments": 0}, st[l]
        assert st[l]["ffn_down"] == ({"state": "refused", "refused_fragments": 1} if l == 1 else {"state": "packed", "refused_fragments": 0}), st[l]
    eng.set_option("w8", 0)
    want = _logits(eng, prompt, toks)
    # eager: every launch of the call is counted; each step launches one FFN down-projection and one paired QKV projection per layer
    for v, per_step in ((1, L - 1), (4, L if qkv else 0), (5, L - 1 + (L if qkv else 0))):
        eng.set_option("w8", v)
        c0 = eng.launch_counts()
        got = _logits(eng, prompt, toks)
        c = _delta(eng.launch_counts(), c0)
        n_down = c["row_gemm_fr1"] // 2
        assert n_down > 0 and n_down % L == 0 and c["w8"] == n_down // L * per_step, (v, c)
        assert np.array_equal(got, want), v


def test_engine_without_the_request_has_no_w8():
    from voicecraft_amd.engine import VoiceCraftEngine
    a, sd, sdq, prompt, toks = _model("tiny128")
    eng = _engine(a, sdq, "none")
    assert eng.options().endswith("|w13=5") and "w8" not in eng.options() and eng.w8_state_dict is None
    assert all(v == {"state": "not_applicable", "refused_fragments": 0} for layer in eng.w8_stats() for v in layer.values())
    for v in (1, 0, 5):
        with pytest.raises(AssertionError):
            eng.set_option("w8", v)
        assert eng.options().endswith("|w13=5")
    c0 = eng.launch_counts()
    _logits(eng, prompt, toks)
    c = _delta(eng.launch_counts(), c0)
    assert c["w8"] == 0 and c["w13"] > 0, c
    assert eng.lib.vc_request_w8(eng._h, 5) == -2          # VC_ESTATE: the request comes before vc_finalize_weights
    for bad in (2, 7, 8, -1):                               # not a mask of 1 | 4: VC_EINVAL, an AssertionError as for every bad input
        cls = type("BadMask", (VoiceCraftEngine,), {"W8_MASK": bad})
        with pytest.raises(AssertionError):
            _engine(a, sdq, "as_is", cls=cls)
    for w8 in ("quantize", "as_is"):                        # the form streams bf16 operands: an fp32 engine refuses the request
        with pytest.raises(AssertionError):
            _engine(a, sdq, w8, dtype="fp32")
    with pytest.raises(AssertionError):
        _engine(a, sdq, "int8")
    eng8 = _engine(a, sdq, "as_is")
    for bad in (2, 7, 8, -1):
        with pytest.raises(AssertionError):
            eng8.set_option("w8", bad)
        assert eng8.options().endswith("|w13=5|w8=5")


def test_w8_free_running_sampled_tokens_equal_option_off():
    """The whole step, sampler included: a sampled call with a seed returns the same tokens with the option on and off."""
    a, sd, sdq, prompt, toks = _model("tiny_h16")
    x, xl, y = prompt
    eng = _engine(a, sd, "quantize")
    out = {}
    for v in (0, 5):
        eng.set_option("w8", v)
        c0 = eng.launch_counts()
        res = eng.inference_tts(x.cuda(), xl.cuda(), y.cuda(), top_k=40, top_p=1.0, temperature=1.0, stop_repetition=3, _seed=1234)
        assert (_delta(eng.launch_counts(), c0)["w8"] > 0) == bool(v)
        out[v] = res[0].cpu().numpy()
    assert out[0].shape == out[5].shape and out[0].shape[-1] > y.shape[1] + 4 and np.array_equal(out[0], out[5])
