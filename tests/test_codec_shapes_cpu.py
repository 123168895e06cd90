"""The codec over the configurations vc_codec_create accepts, the part that needs no GPU (tests/codec_shapes.py lists them):

* the stream geometry (vc_codec_stream_geometry: look-ahead, left context, start frames - derived on the host from kernel
  sizes and ratios) against the transformers.EncodecModel restatement built at the same configuration, by the method of
  tests/test_stream_cpu.py: perturb the codes of frame p / the LSTM output of frame p and read off which frames change;
* the module-index bookkeeping (`expected_keys`, which vc_codec_finalize repeats in C) against the restatement's own names;
* the synthetic weights: they load into the restatement at every configuration, and at the VoiceCraft shape they are the
  tensors the fixed-shape function made before it took a configuration;
* what vc_codec_create refuses before it touches a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import codec_shapes as cs
from oracle import encodec_oracle as eo
from voicecraft_amd import synth
from voicecraft_amd import codec as vcodec

GEOMETRY = dict({k: v for k, v in cs.CONFIGS.items()},
                # (half the filters of the VoiceCraft shape: the geometry does not know the channel count)
                causal=dict(n_filters=32, use_causal_conv=True),
                causal_res3=dict(n_filters=32, use_causal_conv=True, num_residual_layers=3),
                res2_dil3_k7=dict(n_filters=32, num_residual_layers=2, dilation_growth_rate=3, residual_kernel_size=7))


@pytest.fixture(scope="module")
def lib():
    return vcodec._bind(vcodec._lib.load())


@pytest.fixture(scope="module")
def oracles():
    cache = {}

    def get(name):
        if name not in cache:
            cfg = GEOMETRY[name]
            cache[name] = eo.build_cfg(synth.make_codec_state_dict(2, cfg=cfg), cfg)       # (transformers leaves codebooks at zero: the synthetic ones have values)
        return cache[name]
    return get


def _changed_frames(a, b, hop):
    d = (a != b).reshape(-1, hop).any(dim=1)
    return [int(i) for i in d.nonzero().flatten()]


@torch.no_grad()
def _decode_with_lstm_bump(m, codes, p):
    x = m.quantizer.decode(codes.unsqueeze(1))
    for i, layer in enumerate(m.decoder.layers):
        x = layer(x)
        if i == 1 and p >= 0:
            x = x.clone()
            x[:, :, p] += 0.5
    return x[0, 0]


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_geometry_is_sufficient_and_tight_against_the_oracle(name, oracles):
    cfg = dict(vcodec.DEFAULT_CFG, **GEOMETRY[name])
    m = oracles(name)
    hop = int(np.prod(cfg["ratios"]))
    lookahead, left, start = vcodec.stream_geometry(cfg)
    k = cfg["kernel_size"]
    right = lookahead - (0 if cfg["use_causal_conv"] else (k - 1) // 2)        # what is left of it behind the LSTM
    assert lookahead >= 0 and left >= 1 and right >= 0 and start >= 1
    T, p, n_codes = 80, 40, cfg["codebook_size"]
    assert p - lookahead > start and p + left < T - lookahead - 1              # an interior frame: no padding in reach
    g = torch.Generator().manual_seed(11)
    codes = torch.randint(0, n_codes, (cfg["n_q"], T), generator=g)
    base = eo.decode(m, codes)
    assert base.shape == (T * hop,)

    def bump(frame):
        other = codes.clone()
        other[:, frame] = (other[:, frame] + 977) % n_codes                    # 977 is odd and every size here a power of two: another code
        assert (other[:, frame] != codes[:, frame]).all()
        return _changed_frames(base, eo.decode(m, other), hop)
    # ---- look-ahead: the codes of frame p
    ch = bump(p)
    print(name, "codes of frame", p, "changed frames", ch[0], "..", ch[-1], "lookahead", lookahead)
    assert ch[0] >= p - lookahead, (ch[0], lookahead)                          # sufficient
    assert ch[0] == p - lookahead, (ch[0], lookahead)                          # tight to the frame
    # ---- behind the LSTM: the LSTM output of frame p
    ref = _decode_with_lstm_bump(m, codes, -1)
    assert torch.equal(ref, base)
    ch = _changed_frames(ref, _decode_with_lstm_bump(m, codes, p), hop)
    print(name, "LSTM output of frame", p, "reaches frames", ch[0], "..", ch[-1], "left", left, "right", right)
    assert ch[-1] <= p + left - 1 and ch[0] >= p - right, (ch, left, right)    # sufficient
    assert ch[-1] == p + left - 1 and ch[0] == p - right, (ch, left, right)    # tight
    # ---- the true start: once max(start_frames, lookahead + 1) frames are known, frame 0 is final
    first = max(start, lookahead + 1)
    for f in (first, first + 1, first + 5):
        assert 0 not in bump(f), (f, start, lookahead)


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_expected_keys_are_the_restatements_module_names(name, oracles):
    cfg = dict(vcodec.DEFAULT_CFG, **GEOMETRY[name])
    buffers = (".inited", ".cluster_size", ".embed_avg", ".stride", ".kernel_size", ".padding_total")
    got = {k for k in vcodec.normalize_state_dict(oracles(name).state_dict()) if not k.endswith(buffers)}
    want = vcodec.expected_keys(cfg)
    assert got == want, (sorted(got - want)[:5], sorted(want - got)[:5])
    ours = {k for k in vcodec.normalize_state_dict(synth.make_codec_state_dict(0, cfg=GEOMETRY[name])) if not k.endswith(buffers)}
    assert ours == want


@pytest.mark.parametrize("name", list(GEOMETRY))
def test_synthetic_weights_have_the_restatements_shapes(name, oracles):
    """`build` already refuses unexpected keys and missing parameters; here every tensor's shape and value arrived."""
    m = oracles(name)
    sd = synth.make_codec_state_dict(2, cfg=GEOMETRY[name])
    have = m.state_dict()
    for k, t in sd.items():
        assert k in have and tuple(have[k].shape) == tuple(t.shape), (k, tuple(t.shape))
        assert torch.equal(have[k], t), k
    cfg = dict(vcodec.DEFAULT_CFG, **GEOMETRY[name])
    assert len(m.quantizer.layers) == cfg["n_q"]
    assert tuple(m.quantizer.layers[0].codebook.embed.shape) == (cfg["codebook_size"], cfg["hidden"])


def _fixed_shape_codec_state_dict(seed=0, use_conv_shortcut=False, num_residual_layers=1):
    """synth.make_codec_state_dict as it was while it knew one shape only (F = 64, ratios 8/5/4/2, hidden 128, 4 x 2048
    codebooks, a 2-layer LSTM, kernels 7/3/7): the record the configurable function is held to."""
    rs = np.random.RandomState(seed)
    sd = {}

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a).astype(np.float32))

    def conv(prefix, co, ci, k, transposed=False):
        shape = (ci, co, k) if transposed else (co, ci, k)
        fan_in = ci * k if not transposed else ci * k / max(1, k // 2)
        v = rs.standard_normal(size=shape)
        g = np.sqrt((v.reshape(shape[0], -1) ** 2).sum(1)) * (1.4 / np.sqrt(fan_in)) * (0.8 + 0.4 * rs.rand(shape[0]))
        sd[prefix + ".conv.parametrizations.weight.original0"] = t(g.reshape(-1, 1, 1))
        sd[prefix + ".conv.parametrizations.weight.original1"] = t(v)
        sd[prefix + ".conv.bias"] = t(0.05 * rs.standard_normal(size=(co,)))

    def lstm(prefix, h, layers=2):
        for n in range(layers):
            b = h ** -0.5
            sd[f"{prefix}.lstm.weight_ih_l{n}"] = t(rs.uniform(-b, b, size=(4 * h, h)))
            sd[f"{prefix}.lstm.weight_hh_l{n}"] = t(rs.uniform(-b, b, size=(4 * h, h)))
            sd[f"{prefix}.lstm.bias_ih_l{n}"] = t(rs.uniform(-b, b, size=(4 * h,)))
            sd[f"{prefix}.lstm.bias_hh_l{n}"] = t(rs.uniform(-b, b, size=(4 * h,)))

    F, ratios, hidden = 64, [8, 5, 4, 2], 128
    conv("encoder.layers.0", F, 1, 7)
    idx, ch = 1, F

    def res_unit(prefix, dim):
        conv(prefix + ".block.1", dim // 2, dim, 3)
        conv(prefix + ".block.3", dim, dim // 2, 1)
        if use_conv_shortcut:
            conv(prefix + ".shortcut", dim, dim, 1)

    for r in reversed(ratios):
        for _ in range(num_residual_layers):
            res_unit(f"encoder.layers.{idx}", ch)
            idx += 1
        idx += 1
        conv(f"encoder.layers.{idx}", ch * 2, ch, 2 * r)
        idx += 1
        ch *= 2
    lstm(f"encoder.layers.{idx}", ch)
    idx += 2
    conv(f"encoder.layers.{idx}", hidden, ch, 7)
    conv("decoder.layers.0", ch, hidden, 7)
    lstm("decoder.layers.1", ch)
    idx = 2
    for r in ratios:
        idx += 1
        conv(f"decoder.layers.{idx}", ch // 2, ch, 2 * r, transposed=True)
        idx += 1
        for _ in range(num_residual_layers):
            res_unit(f"decoder.layers.{idx}", ch // 2)
            idx += 1
        ch //= 2
    idx += 1
    conv(f"decoder.layers.{idx}", 1, F, 7)
    for q in range(4):
        sd[f"quantizer.layers.{q}.codebook.embed"] = t(rs.standard_normal(size=(2048, hidden)) * (0.6 ** q))
    return sd


@pytest.mark.parametrize("seed,kw", [(0, {}), (2, dict(use_conv_shortcut=True)), (2, dict(num_residual_layers=2))])
def test_default_shape_tensors_are_unchanged(seed, kw):
    """Every existing codec test and fixture draws its weights from this function: same generator, same draw order."""
    want = _fixed_shape_codec_state_dict(seed, **kw)
    for got in (synth.make_codec_state_dict(seed, **kw), synth.make_codec_state_dict(seed, cfg=dict(vcodec.DEFAULT_CFG, **kw))):
        assert list(got) == list(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k


REFUSED = [("ratios", dict(ratios=[8, 5, 4, 1])), ("ratios", dict(ratios=[0, 2])), ("ratios", dict(ratios=[2, -3])),
           ("lstm_layers", dict(lstm_layers=0)), ("lstm_layers", dict(lstm_layers=-1)),
           ("codebook_size", dict(codebook_size=0)), ("codebook_size", dict(codebook_size=-16)),
           ("hidden", dict(hidden=0)), ("hidden", dict(hidden=-16)), ("hidden", dict(hidden=8)), ("hidden", dict(hidden=40)),
           ("n_filters", dict(n_filters=0)), ("n_filters", dict(n_filters=-32)), ("n_filters", dict(n_filters=16)),
           ("n_filters", dict(n_filters=48)),
           ("kernel_size", dict(kernel_size=0)), ("kernel_size", dict(kernel_size=-7)),
           ("residual_kernel_size", dict(residual_kernel_size=0)), ("last_kernel_size", dict(last_kernel_size=0)),
           ("last_kernel_size", dict(last_kernel_size=-1)),
           ("n_ratios", dict(ratios=[])), ("n_ratios", dict(ratios=[2] * 9)), ("n_q", dict(n_q=0)), ("n_q", dict(n_q=9)),
           ("num_residual_layers", dict(num_residual_layers=0)), ("dilation_growth_rate", dict(dilation_growth_rate=5))]


@pytest.mark.parametrize("field,kw", REFUSED, ids=[f"{f}-{i}" for i, (f, _) in enumerate(REFUSED)])
def test_create_refuses_what_the_engine_cannot_run(lib, field, kw):
    """vc_codec_create validates before it touches HIP: VC_EINVAL, no handle, and a message that names the field."""
    ratios = kw.get("ratios", vcodec.DEFAULT_CFG["ratios"])
    cfg = vcodec.make_cfg(dict(kw, ratios=ratios[:vcodec.VC_CODEC_MAX_RATIOS]), max_samples=16000)
    cfg.n_ratios = len(ratios)
    h = C.c_void_p()
    assert lib.vc_codec_create(C.byref(cfg), 0, C.byref(h)) == -1
    assert not h.value
    msg = lib.vc_codec_last_error(None).decode()
    assert field in msg, msg


def test_create_refusals_do_not_hide_behind_one_another(lib):
    """max_samples / max_batch / compress keep their messages, and a NULL config or result pointer is VC_EINVAL."""
    h = C.c_void_p()
    for field, setter in (("max_samples", lambda c: setattr(c, "max_samples", 0)), ("max_batch", lambda c: setattr(c, "max_batch", 65)),
                          ("compress", lambda c: setattr(c, "compress", 4))):
        cfg = vcodec.make_cfg(max_samples=16000)
        setter(cfg)
        assert lib.vc_codec_create(C.byref(cfg), 0, C.byref(h)) == -1 and not h.value
        assert field in lib.vc_codec_last_error(None).decode()
    assert lib.vc_codec_create(None, 0, C.byref(h)) == -1
    assert lib.vc_codec_create(C.byref(vcodec.make_cfg()), 0, None) == -1
    a, b = C.c_int(0), C.c_int(0)
    assert lib.vc_codec_last_forms(None, C.byref(a), C.byref(b)) == -1


@pytest.mark.parametrize("name", list(cs.CONFIGS))
def test_the_oracle_takes_the_wanted_number_of_quantizers(name):
    """transformers derives n_q from a bandwidth; overrides_from_cfg computes the bandwidth that yields it."""
    from transformers import EncodecConfig
    cfg = cs.full(name)
    c = EncodecConfig(**dict(dict(audio_channels=1, normalize=False, chunk_length_s=None, norm_type="weight_norm"),
                             **eo.overrides_from_cfg(cs.CONFIGS[name])))
    assert c.num_quantizers == cfg["n_q"] and c.hop_length == cs.hop_of(name)
    assert c.codebook_size == cfg["codebook_size"] and c.hidden_size == cfg["hidden"] == c.codebook_dim
