"""Option `kv8` (an E4M3 copy of the K / V cache, voicecraft_amd/csrc/vc_kv8.h): what the CPU and the GPU tests share.  No GPU here.

* an independent numpy statement of the grid (the 127 E4M3 magnitudes by enumeration, nearest by search, ties to the even code) and the
  rows the quantiser is held to;
* the test oracle: VoiceCraftOracle whose cached attention reads the PAST rows through the quantiser's round trip of their bf16 values
  and the rows of the current pass as they are - the contract of the option;
* the kernel-level cases: launches of tests/decode_attn_cases.py turned into passes of `rps` rows per sequence."""
from __future__ import annotations

import numpy as np
import torch

import decode_attn_cases as dc
from oracle.voicecraft_oracle import VoiceCraftOracle

SHIFT_MIN, SHIFT_MAX = -117, 119
HDS = (32, 64, 128)


# ------------------------------------------------------------------------------------------------ the grid, stated apart from quant.py
def e4m3_magnitudes() -> np.ndarray:
    """Magnitude of code c = 0 .. 126 (0x7f is the NaN code), float64, increasing."""
    out = []
    for code in range(0x7f):
        e, m = code >> 3, code & 7
        out.append(m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
    out = np.array(out)
    assert (np.diff(out) > 0).all()
    return out


E4M3 = e4m3_magnitudes()


def grid_shift(row: np.ndarray) -> int:
    """floor(log2 amax) - 8, clamped; one more where amax * 2^-s > 464; a row of zeros takes 0."""
    amax = float(np.abs(row.astype(np.float64)).max())
    if amax == 0:
        return 0
    s = int(np.clip(int(np.floor(np.log2(amax))) - 8, SHIFT_MIN, SHIFT_MAX))
    if amax * 2.0 ** -s > 464.0:
        s += 1
    return min(s, SHIFT_MAX)


def grid_quantize(rows: np.ndarray):
    """rows [n][hd] (bf16-valued) -> (codes uint8 [n][hd], shift int8 [n]) by search over the enumerated magnitudes."""
    rows = np.asarray(rows, dtype=np.float64)
    codes = np.zeros(rows.shape, dtype=np.uint8)
    shift = np.zeros(rows.shape[0], dtype=np.int8)
    for i, r in enumerate(rows):
        s = grid_shift(r)
        x = np.minimum(np.abs(r) * 2.0 ** -s, 448.0)
        hi = np.clip(np.searchsorted(E4M3, x), 1, 126)              # E4M3[hi - 1] <= x <= E4M3[hi] (x <= 448 = E4M3[126])
        lo = hi - 1
        dl, dh = x - E4M3[lo], E4M3[hi] - x
        c = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
        codes[i] = c.astype(np.uint8) | np.where(np.signbit(r), 0x80, 0).astype(np.uint8)
        shift[i] = s
    return codes, shift


def grid_values(codes: np.ndarray, shift: np.ndarray) -> np.ndarray:
    mag = E4M3[codes & 0x7f] * 2.0 ** shift.astype(np.float64)[..., None]
    return np.where(codes & 0x80, -mag, mag)


def bf16(x) -> torch.Tensor:
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).bfloat16().float()


def next_bf16_up(v: float) -> float:
    b = torch.tensor([v], dtype=torch.float32).bfloat16().view(torch.int16)
    return float((b + 1).view(torch.bfloat16).float())


def special_rows(hd: int) -> torch.Tensor:
    """The rows the issue names: zeros, +-0, one huge value among tiny ones, maxima at exactly 448 . 2^s, 464 . 2^s and the next bf16 above
    it (at several binades), values at rounding ties in the normal and the denormal range, and the ends of the shift range."""
    rows = []
    g = torch.Generator().manual_seed(hd)

    def row(fill=0.0):
        return torch.full((hd,), float(fill))

    rows.append(row())                                               # zeros
    r = row(); r[1::2] = -0.0; rows.append(r)                        # +-0
    r = bf16(torch.randn(hd, generator=g) * 2.0 ** -20); r[3] = 3.0e4; rows.append(r)      # one huge value among tiny ones
    r = bf16(torch.randn(hd, generator=g) * 2.0 ** -20); r[5] = -1.0; r[6] = 2.0 ** -18; r[7] = -1.5 * 2.0 ** -17; rows.append(r)
    for s0 in (-20, -9, 0, 5, 30):
        for top in (448.0, 464.0, next_bf16_up(464.0), 256.0, 254.0, 480.0, 510.0):
            r = bf16(torch.randn(hd, generator=g).clamp(-1, 1) * 200.0 * 2.0 ** s0)
            r[0] = top * 2.0 ** s0
            r[1] = -top * 2.0 ** s0
            # ties: odd sixteenths of a binade (17/16, 19/16 -> 16/16, 20/16: even mantissa), 2.5 and 3.5 denormal steps, half the smallest step
            r[2:6] = torch.tensor([272.0, 304.0, -272.0, -304.0]) * 2.0 ** s0
            r[6:10] = torch.tensor([2.5, 3.5, -2.5, -3.5]) * 2.0 ** (s0 - 9)
            r[10:14] = torch.tensor([0.5, 1.5, -0.5, 0.4]) * 2.0 ** (s0 - 9)
            r[14] = 2.0 ** (s0 - 6)                                   # the bottom of the normal range
            r[15] = 7.5 * 2.0 ** (s0 - 9)                             # the tie between the last denormal and the first normal code
            rows.append(bf16(r))
    rows.append(bf16(torch.randn(hd, generator=g) * 2.0 ** -122))     # below the smallest shift's normal range
    rows.append(bf16(torch.randn(hd, generator=g).clamp(-3, 3) * 2.0 ** 124))
    out = bf16(torch.stack(rows))
    assert bool(torch.isfinite(out).all()) and bool((out == out.bfloat16().float()).all())
    return out


def random_rows(hd: int, n: int = 4096, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(1000 * seed + hd)
    scale = torch.exp2(torch.randint(-12, 6, (n, 1), generator=g).float())
    spread = torch.exp2(torch.randint(-14, 1, (n, hd), generator=g).float())
    return bf16(torch.randn(n, hd, generator=g) * scale * spread)


# ------------------------------------------------------------------------------------------------ the test oracle
class Kv8Oracle(VoiceCraftOracle):
    """The plain oracle, except that the cached rows a step attends to are read through `roundtrip` of their bf16 values (default: the
    kv8 quantiser's); the rows of the step itself are left alone."""

    def __init__(self, *a, roundtrip=None, **k):
        super().__init__(*a, **k)
        if roundtrip is None:
            from voicecraft_amd import quant
            roundtrip = lambda t: quant.kv8_roundtrip(t.bfloat16().float())
        self.roundtrip = roundtrip

    def _attn(self, l, x, mask, past_l):
        if past_l is not None:
            past_l = self.roundtrip(past_l).to(past_l.dtype)
        return super()._attn(l, x, mask, past_l)


def cached_tts_logits(orc, prompt, toks) -> np.ndarray:
    """Head logits [steps][K][V] of the oracle's CACHED path (kvcache = 1) along the forced trajectory."""
    x, xl, y = prompt
    tr = []
    orc.inference_tts(x, xl, y, top_k=1, kvcache=1, trace=tr, forced=toks)
    return torch.stack([t["logits"][0] for t in tr]).numpy()


def cached_edit_logits(orc, x, xl, y, spans, toks) -> np.ndarray:
    tr = []
    orc.inference(x, xl, y, torch.tensor([spans]), top_k=1, kvcache=1, trace=tr, forced=toks)
    return torch.stack([t["logits"][0] for t in tr]).numpy()


# ------------------------------------------------------------------------------------------------ kernel-level cases
PPW8 = {hd: 64 * 16 // hd for hd in HDS}          # positions a wave reads per request on the E4M3 cache


def batch8(hd):
    return 4 * dc.NW * PPW8[hd]


def pass_lengths(hd, nsplit, rps):
    """Context lengths S of the LAST row of each sequence of a pass: around every edge of the kv8 partition - the positions per visit, the
    batch, the refill of an n-way split - so that tails of 1..rps rows straddle split and batch edges."""
    P, B = PPW8[hd], batch8(hd)
    s = {rps, rps + 1, nsplit + rps, P - 1 + rps, P + 1, P + rps, 8 * P + 1, B, B + 1, B + rps - 1, B + rps, nsplit * B, nsplit * B + 1,
         nsplit * B + rps, 2 * B + 1, dc.MAX_NSPLIT * B + 1 if nsplit == dc.MAX_NSPLIT else B + 2}
    for S in range(nsplit + rps, 4 * nsplit + rps + 8):      # a split edge inside the tail: (S - rps .. S) straddles a chunk boundary
        c = int(dc.chunk_rule(S, nsplit))
        if any(S - rps < e < S for e in range(c, S, c)):
            s.add(S)
    return sorted(x for x in s if x >= rps)
