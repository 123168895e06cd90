"""The 13-bit weight planes of option `w13` (voicecraft_amd/csrc/vc_w13.h), without a GPU.

* tools/w13_check.cpp - a stand-alone program around the header's encode / decode, built with the host compiler and
  -fsanitize=address,undefined - round-trips all 65 536 bf16 bit patterns placed in fragments, fragments of zeros, +-0 mixes and
  denormals, a full 30-binade span at every position of the window, and refuses (never mis-encodes) a fragment one step too wide.
* A numpy restatement of the packer's acceptance rule over the weights the benchmark runs on (giga830M, seed 0, layer 0) and over
  the trained-statistics checkpoints: no fragment of the two converted matrices (FFN-down, QKV) is refused, i.e. the benchmark and those tests really
  run the packed form."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_round_trip_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "w13_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", str(exe), os.path.join(ROOT, "tools", "w13_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    word, frags, refused = r.stdout.split()
    assert word == "ok" and int(frags) > 2000 and int(refused) > 0, r.stdout


# ---- the acceptance rule, restated: a 512-value fragment is refused when its non-zero hi7 = bits 14..8 span more than 15 steps
def bf16_bits(w: torch.Tensor, colscale=None) -> np.ndarray:
    """The bf16 image's values: W (. gamma, in fp32, for a matrix behind a LayerNorm) rounded to nearest even."""
    if colscale is not None:
        w = w * colscale[None, :]
    return w.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def refused_fragments(bits: np.ndarray, th: int, kw: int) -> tuple:
    """(fragments, refused, values with hi7 = 0) of an [N, K] matrix in tiles of `th` channels x `kw` consecutive k (8 x 64: the one-row
    paired kernel's fragment pairs)."""
    N, K = bits.shape
    assert N % th == 0 and K % kw == 0
    hi7 = ((bits >> 8) & 0x7f).astype(np.int16).reshape(N // th, th, K // kw, kw).transpose(0, 2, 1, 3).reshape(-1, th * kw)
    assert hi7.shape[1] == 512
    mx = hi7.max(axis=1)
    mn = np.where(hi7 == 0, 128, hi7).min(axis=1)
    refused = (mx > 0) & (mx - mn >= 15)
    return hi7.shape[0], int(refused.sum()), int((hi7 == 0).sum())


def layer_fragments(sd, l: int) -> tuple:
    p = f"decoder.layers.{l}."
    out = [refused_fragments(bf16_bits(sd[p + "linear2.weight"]), 8, 64),
           refused_fragments(bf16_bits(sd[p + "self_attn.in_proj_weight"], sd[p + "norm1.weight"]), 8, 64)]
    return tuple(sum(o[i] for o in out) for i in range(3))


def test_bench_weights_layer0_has_no_refused_fragment():
    from voicecraft_amd import synth
    a = synth.make_args("giga830M", num_decoder_layers=1)
    sd = synth.make_state_dict(a, seed=0, fast=True)
    n, refused, zeros = layer_fragments(sd, 0)
    print(f"giga830M layer 0: {n} fragments, {refused} refused, {zeros} values with hi7 = 0")
    assert n == (2048 // 8) * (8192 // 64) + (6144 // 8) * (2048 // 64) and refused == 0


@pytest.mark.parametrize("preset", ["tiny128", "tiny_h16"])
@pytest.mark.parametrize("setting", ["A", "B"])
def test_trained_stats_checkpoints_have_no_refused_fragment(preset, setting):
    import trained_stats_cases as C
    a, sd, _ = C.checkpoint(preset, C.stats_key(setting, bf16=True))
    tot = [0, 0]
    for l in range(a.num_decoder_layers):
        n, refused, _ = layer_fragments(sd, l)
        tot[0] += n; tot[1] += refused
    print(f"{preset} {setting}: {tot[0]} fragments, {tot[1]} refused")
    assert tot[0] == a.num_decoder_layers * (2048 + 1536) and tot[1] == 0


def test_rule_refuses_a_stray_tiny_value():
    """1.0 next to 1e-12 (40 binades apart) in one fragment refuses that fragment and no other."""
    w = torch.full((16, 128), 0.02)
    w[3, 70] = 1.0
    w[4, 71] = 1e-12
    assert refused_fragments(bf16_bits(w), 8, 64) == (4, 1, 0)
    w[4, 71] = 0.0          # an exact zero is code 0: not part of the span
    assert refused_fragments(bf16_bits(w), 8, 64) == (4, 0, 1)
