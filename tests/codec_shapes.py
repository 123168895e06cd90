"""Codec configurations other than the VoiceCraft shape, and the bars every codec comparison against the
transformers.EncodecModel restatement uses - shared by tests/test_codec_shapes_cpu.py and tests/test_gpu_codec_shapes.py.

A configuration is the dict `AudioTokenizer(cfg=...)` takes (names of `voicecraft_amd.codec.DEFAULT_CFG`); the same dict makes
the synthetic weights (`synth.make_codec_state_dict(cfg=...)`) and the oracle (`encodec_oracle.build_cfg`).  Each row turns
several knobs at once so that together every kernel form and branch of vc_codec.hip runs:

  id        n_filters  ratios (hop)      LSTM H, layers  hidden  n_q x C    kernels first/res/last
  half      32         8,5,4,2 (320)     512, 2          64      8 x 1024   7/3/7   lstm_persist_k<2>, lstm_wave_k<2>, 16-channel residual conv, nks 4
  narrow    32         4,4,2 (32)        256, 2          48      2 x 16     5/5/3   lstm_wave_k<1> (no persistent form), 3-tile last conv, nks 3, one-tile codebook
  w768      96         5,3,2 (30)        768, 2          128     3 x 8      7/3/7   lstm_wave_k<3>, 48-channel residual convs, ratio 3, scalar RVQ (C % 16)
  seq       32         2,2 (4)           128, 1          272     5 x 64     7/3/7   lstm_step_k, scalar RVQ (D > 256), stride-2-only stack
  even      32         2,2,2,2,2 (32)    1024, 2         256     1 x 2048   4/2/6   five ratios, even kernel sizes, nks 16, n_q 1
  fullsize  64         8,5,4,2 (320)     1024, 2         128     4 x 2048   7/3/7   max_seconds 2.01 (no hop multiple): 32160 samples <-> 101 frames
  seq3      32         4,2 (8)           256, 3          32      3 x 32     7/3/7   three LSTM layers through lstm_step_k, nks 2, a two-tile codebook; no stream
"""
import math

import numpy as np
import torch

SR = 16000

CONFIGS = {
    "half": dict(n_filters=32, ratios=[8, 5, 4, 2], hidden=64, n_q=8, codebook_size=1024),
    "narrow": dict(n_filters=32, ratios=[4, 4, 2], hidden=48, n_q=2, codebook_size=16, kernel_size=5,
                   residual_kernel_size=5, last_kernel_size=3),
    "w768": dict(n_filters=96, ratios=[5, 3, 2], hidden=128, n_q=3, codebook_size=8),
    "seq": dict(n_filters=32, ratios=[2, 2], lstm_layers=1, hidden=272, n_q=5, codebook_size=64),
    "even": dict(n_filters=32, ratios=[2, 2, 2, 2, 2], hidden=256, n_q=1, codebook_size=2048, kernel_size=4,
                 residual_kernel_size=2, last_kernel_size=6),
    "fullsize": dict(),
    "seq3": dict(n_filters=32, ratios=[4, 2], lstm_layers=3, hidden=32, n_q=3, codebook_size=32),
}
SEED = {"half": 0, "narrow": 0, "w768": 0, "seq": 0, "even": 0, "fullsize": 0, "seq3": 0}      # of the synthetic weights
MAX_BATCH = {"half": 2, "narrow": 3}                                                          # 1 elsewhere
# (lstm_form, rvq_form) the row must reach by default (vc_codec_last_forms): LSTM 0 step kernels / 1 wavefront / 2 persistent
FORMS = {"half": (2, 1), "narrow": (1, 1), "w768": (1, 0), "seq": (0, 0), "even": (2, 1), "fullsize": (2, 1), "seq3": (0, 1)}


def full(name):
    from voicecraft_amd.codec import DEFAULT_CFG
    return dict(DEFAULT_CFG, **CONFIGS[name])


def hop_of(name):
    return math.prod(full(name)["ratios"])


def max_seconds(name):
    """fullsize: 2.01 s = 32160 samples = 100.5 frames.  Elsewhere room for the 130-frame clips and no more."""
    return 2.01 if name == "fullsize" else 131 * hop_of(name) / SR


def decode_lengths(name):
    return [101] if name == "fullsize" else [1, 3, 40, 130]


def encode_lengths(name):
    h = hop_of(name)
    return [40 * h + 3, 32160, h + 1] if name == "fullsize" else [40 * h + 3, 130 * h, h + 1]


def random_codes(name, T, seed=None):
    cf = full(name)
    rs = np.random.RandomState(T if seed is None else seed)
    return torch.from_numpy(rs.randint(0, cf["codebook_size"], size=(cf["n_q"], T)).astype(np.int64))


def random_wav(n, B=1):
    g = torch.Generator().manual_seed(n)
    return torch.randn(B, 1, n, generator=g) * 0.1


# ---------------------------------------------------------------------------------------------- the project's bars
LATENT_BAR = 1e-3          # relative L2 of the latent in front of the quantizer


def wave_bar(want):
    """max |d| allowed on a waveform: 2e-4 of the signal's RMS + 1e-5"""
    return 2e-4 * float(np.sqrt((np.asarray(want, dtype=np.float64) ** 2).mean())) + 1e-5


def latent_error(z, z_o):
    return float((z.double() - z_o.double()).norm() / z_o.double().norm())


def check_codes(codes, codes_o, z, z_o, codebooks):
    """The code bar of test_encode_matches_oracle: every frame whose codes differ must sit, at the FIRST stage where they
    differ, on a near-tie of the oracle's own search (gap of the two squared distances <= 8 * err * (|r| + 1), err = the
    largest latent error), and the disagreeing (stage, frame) cells are at most max(1, 1 %) of all cells (clips of fewer
    than 9 frames are exempt from the count, not from the near-tie rule).  -> (cells that differ, cells)"""
    assert codes.shape == codes_o.shape, (codes.shape, codes_o.shape)
    Q, T = codes_o.shape
    z, z_o = z.double(), z_o.double()
    E = [e.double() for e in codebooks]
    err = float((z - z_o).abs().max())
    for t in (codes != codes_o).any(dim=0).nonzero().flatten().tolist():
        r = z_o[t].clone()
        for q in range(Q):
            d = ((r[None] - E[q]) ** 2).sum(1)
            if codes[q, t] != codes_o[q, t]:
                gap = float(d[codes[q, t]] - d[codes_o[q, t]])
                assert gap <= 8 * err * float(r.norm() + 1), (t, q, gap, err)
                break
            r = r - E[q][codes_o[q, t]]
    bad = int((codes != codes_o).sum())
    if T >= 9:
        assert bad <= max(1, (Q * T) // 100), (bad, Q * T)
    return bad, Q * T


def oracle_codebooks(m):
    return [layer.codebook.embed for layer in m.quantizer.layers]
