"""Puts a checkpoint on the engine's 8-bit weight grid ("w8", csrc/vc_w8.h), on the CPU; at the end of the file the CPU statement of the
same grid for cached K / V rows ("kv8", csrc/vc_kv8.h).

The grid's unit is the 512-value MFMA fragment of the engine's 8-channel-tile images: an aligned block of 8 output channels x 64
inputs of the bf16 image (csrc/vc_gemm.hip pack_k with th = 8: a tile is 8 channels x 32 inputs, a fragment two consecutive
k-tiles).  A block is on the grid when one shift s exists with every value = q * 2**s, q an OCP E4M3 number (float8_e4m3fn, never its
NaN code) and the value a normal bf16 number or +-0.  The result is an ordinary fp32 state dict: the oracle and every engine path run
on it unchanged, and an engine created with `w8="as_is"` on it (or `w8="quantize"` on the original) streams the named matrices of
one-row steps as one byte per value, with results bit-identical to the bf16 launches on the same state dict.

What lands on the grid is the engine's IMAGE, not the stored matrix: bf16(W) for `linear2.weight`; bf16(W * gamma), the fp32 product
with gamma = norm1.weight rounded to nearest even, for `self_attn.in_proj_weight` (the LayerNorm fold, csrc/vc_gemm.hip).  The folded
matrix Q is quantised, Q / gamma is returned, and the fold of the result is asserted to reproduce Q element by element.  On request
(`ffn_up=True`, engine option `w8u`) the FFN up-projection joins them the same way: bf16(linear1.weight * norm2.weight)."""
from __future__ import annotations

import torch

BLOCK = (8, 64)                 # output channels x inputs of one fragment
SHIFT_MIN, SHIFT_MAX = -117, 119
MATRICES = {"ffn_down": ("linear2.weight", None), "qkv": ("self_attn.in_proj_weight", "norm1.weight")}
# the third matrix, by the keyword `ffn_up=True` only (`matrices` keeps naming the two the one-row planes exist for): the 16-channel
# image of wide steps, whose pairs are two blocks of the same grid each (w8w_decode below)
FFN_UP = ("linear1.weight", "norm2.weight")


def _blocks(x: torch.Tensor) -> torch.Tensor:
    n, k = x.shape
    bn, bk = BLOCK
    assert n % bn == 0 and k % bk == 0, f"matrix [{n}, {k}] is not whole {bn} x {bk} blocks"
    return x.reshape(n // bn, bn, k // bk, bk).permute(0, 2, 1, 3).reshape(n // bn, k // bk, bn * bk)


def _unblocks(b: torch.Tensor, n: int, k: int) -> torch.Tensor:
    bn, bk = BLOCK
    return b.reshape(n // bn, k // bk, bn, bk).permute(0, 2, 1, 3).reshape(n, k)


def block_shifts(image: torch.Tensor) -> torch.Tensor:
    """The shift of every block of a bf16-valued fp32 matrix: emax - 8 puts the block's largest value into E4M3's top binade
    (256 .. 448).  A maximum above 464 * 2**s - past the midpoint between 448 and the NaN code 480 - takes one shift more, where 480 and
    512 exist (240, 256); clamping it to 448 would cost up to an eighth of the value.  Blocks of zeros take 0."""
    amax = _blocks(image).abs().amax(dim=-1).double()
    _, e = torch.frexp(amax)                                  # amax = m * 2**e, m in [0.5, 1)
    s = (e - 1 - 8).clamp(SHIFT_MIN, SHIFT_MAX)
    s = torch.where(torch.ldexp(amax, -s) > 464.0, s + 1, s)
    assert int(s.max()) <= SHIFT_MAX, "a block's largest value does not fit the grid's last shift"
    return torch.where(amax == 0, torch.zeros_like(s), s)


def quantize_image(image: torch.Tensor) -> torch.Tensor:
    """A bf16-valued fp32 matrix -> the nearest matrix (ties to even) on the grid, block by block.  Values beyond 448 * 2**s are clamped
    (torch's float8 cast turns them into NaN), values below half the smallest denormal 2**(s - 9) become +-0."""
    assert image.dtype == torch.float32 and bool(torch.isfinite(image).all())
    n, k = image.shape
    b = _blocks(image).double()
    s = block_shifts(image).unsqueeze(-1)
    x = torch.ldexp(b, -s).clamp(-448.0, 448.0).float()       # exact: a power-of-two scaling of bf16 values (tiny ones may flush to 0)
    q = x.to(torch.float8_e4m3fn).float().double()
    out = _unblocks(torch.ldexp(q, s), n, k).float()
    assert bool(torch.isfinite(out).all())
    assert bool((out == out.bfloat16().float()).all()), "grid values are bf16 numbers"
    return out


def fold(w: torch.Tensor, gamma: torch.Tensor | None) -> torch.Tensor:
    """The engine's bf16 image of a matrix as fp32 values: the fp32 product with the LayerNorm weight, column by column, rounded to nearest
    even (pack_k: `v *= colscale[k]`, then f32 -> bf16)."""
    w = w.detach().to(torch.float32)
    if gamma is not None:
        w = w * gamma.detach().to(torch.float32)[None, :]
    return w.bfloat16().float()


def quantize_matrix(w: torch.Tensor, gamma: torch.Tensor | None = None) -> torch.Tensor:
    """The fp32 matrix to store so that the engine's image of it lies on the grid.  Behind a LayerNorm: quantises Q = bf16(W * gamma)
    and returns Q / gamma; columns with gamma = 0 (image column of zeros, on every grid) are left alone."""
    img = fold(w, gamma)
    q = quantize_image(img)
    if gamma is None:
        return q
    g = gamma.detach().to(torch.float32)
    live = g != 0
    out = w.detach().to(torch.float32).clone()
    out[:, live] = (q[:, live].double() / g[live].double()[None, :]).float()
    # fp32(Q / gamma) * gamma = Q (1 + d) with |d| < 2**-22, and Q is a bf16 number: the rounding to bf16 gives Q back unless the quotient
    # or the product leaves fp32's normal range
    again = fold(out, g)
    assert bool((again == q).all()), f"{int((again != q).sum())} folded values left the grid (a LayerNorm weight outside fp32's normal range?)"
    return out


def quantize_state_dict_w8(args, sd: dict, matrices=("ffn_down", "qkv"), ffn_up: bool = False) -> dict:
    """A new fp32 state dict whose named matrices (of every decoder layer) lie on the w8 grid; every other tensor is the input's, cloned.
    ffn_up: also the FFN up-projection, folded with norm2.weight (what an engine created with `w8_up=True` streams at 17..64 rows).
    Idempotent: a second pass changes nothing."""
    unknown = [m for m in matrices if m not in MATRICES]
    assert not unknown, f"unknown matrices {unknown}: {sorted(MATRICES)} exist"
    out = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in sd.items()}
    n_layers = int(args["num_decoder_layers"] if isinstance(args, dict) else args.num_decoder_layers)
    for l in range(n_layers):
        p = f"decoder.layers.{l}."
        for m in matrices:
            wkey, gkey = MATRICES[m]
            gamma = sd[p + gkey] if gkey else None
            out[p + wkey] = quantize_matrix(sd[p + wkey], gamma).to(torch.float32)
        if ffn_up:
            wkey, gkey = FFN_UP
            out[p + wkey] = quantize_matrix(sd[p + wkey], sd[p + gkey]).to(torch.float32)
    return out


# ---- "w8w": the pair planes of the 16-channel images that 17..64-row steps stream (csrc/vc_w8.h) ----------------------------------------
def w8w_decode(planes: torch.Tensor, side: torch.Tensor) -> torch.Tensor:
    """The stated layout of a pair, read back: planes uint8 [n_pairs, 1024] - 16 bytes per lane, lane l's eight codes of k-tile 2j then its
    eight of k-tile 2j + 1 - and side uint8 [n_pairs, 2] - shift + 127 of channels 0..7 (lanes with l & 8 == 0), of channels 8..15 ->
    fp32 [n_pairs, 2, 64, 8]: k-tile of the pair, lane, value (lane l = channel l & 15 of the tile, inputs 8 (l >> 4) .. + 7 of the
    k-tile).  A pair is two BLOCK-shaped blocks of the grid above: channels 0..7 x 64 inputs and channels 8..15 x 64 inputs."""
    n = planes.shape[0]
    q = planes.contiguous().view(torch.float8_e4m3fn).float().double().reshape(n, 64, 2, 8).permute(0, 2, 1, 3)
    half = (torch.arange(64) >> 3) & 1
    shift = side.to(torch.int32)[:, half] - 127                      # [n_pairs, 64]
    return torch.ldexp(q, shift[:, None, :, None]).float()


# ---- "w8q": the pairs of the 12-channel QKV image that finished-row passes stream (csrc/vc_w8.h) ---------------------------------------
def w8q_decode(planes: torch.Tensor, side: torch.Tensor, kt: int) -> torch.Tensor:
    """The stated layout of a pair, read back: planes uint8 [n_pairs, 768] - 16 bytes per slot, slot s = kg * 12 + m (channel m of the
    tile, inputs 8 kg .. + 7 of a k-tile) holding its eight codes of k-tile 2j then its eight of k-tile 2j + 1 - and side uint8
    [n_pairs, 2] - shift + 127 of part 0, of part 1 -> fp32 [n_pairs, 2, 48, 8]: k-tile of the pair, slot, value.  kt = k-tiles per tile:
    pair P belongs to tile P // (kt // 2).  The parts split a tile's 12 channels at the quantiser's 8-channel block boundary: an even
    tile's part 1 is m >= 8, an odd tile's m >= 4."""
    n = planes.shape[0]
    q = planes.contiguous().view(torch.float8_e4m3fn).float().double().reshape(n, 48, 2, 8).permute(0, 2, 1, 3)
    m = torch.arange(48) % 12
    odd = ((torch.arange(n) // (kt // 2)) & 1).bool()
    part = torch.where(odd[:, None], m[None, :] >= 4, m[None, :] >= 8).long()          # [n_pairs, 48]
    shift = torch.gather(side.to(torch.int32), 1, part) - 127
    return torch.ldexp(q, shift[:, None, :, None]).float()


# ---- "kv8": cached K / V rows on the same grid, the block being one head's row of hd values (csrc/vc_kv8.h) -----------------------------
def kv8_quantize_rows(x: torch.Tensor):
    """bf16-valued rows [..., hd] -> (codes uint8 [..., hd], shift int8 [...]): value ~ q * 2**shift, q the float8_e4m3fn number the code
    byte holds.  The shift is block_shifts' rule with the row as the block (floor(log2 amax) - 8, clamped to the range, one more where
    amax * 2**-s > 464, 0 for a row of zeros); values are scaled, clamped to +-448 and rounded to nearest even, so the NaN code is never
    stored.  This is the statement the engine's packer (kv8_pack_k) must match bit for bit."""
    x = x.detach().to(torch.float32)
    assert bool(torch.isfinite(x).all()) and bool((x == x.bfloat16().float()).all()), "rows of finite bf16 values"
    amax = x.abs().amax(dim=-1).double()
    _, e = torch.frexp(amax)
    s = (e - 1 - 8).clamp(SHIFT_MIN, SHIFT_MAX)
    s = torch.where(torch.ldexp(amax, -s) > 464.0, s + 1, s).clamp(max=SHIFT_MAX)
    s = torch.where(amax == 0, torch.zeros_like(s), s)
    q = torch.ldexp(x.double(), -s.unsqueeze(-1)).clamp(-448.0, 448.0).float()
    codes = q.to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, s.to(torch.int8)


def kv8_dequantize(codes: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """The fp32 values (bf16 numbers, all of them) the codes stand for at their rows' shifts."""
    q = codes.contiguous().view(torch.float8_e4m3fn).float().double()
    return torch.ldexp(q, shift.to(torch.int32).unsqueeze(-1)).float()


def kv8_roundtrip(x: torch.Tensor) -> torch.Tensor:
    """What a kv8 engine's decode attention reads in place of the cached rows x [..., hd]."""
    return kv8_dequantize(*kv8_quantize_rows(x))


# ---- "kv8c": centred K (csrc/vc_kv8.h states the contract; this is its restatement) ---------------------------------------------------
# The centre.  For every layer, cache slot and head there is a bf16 vector c[hd]: the mean of the slot's bf16 K rows at positions
#   0 .. n0-1, accumulated in fp32 and rounded to bf16; n0 = the rows of that sequence in the prefill pass that wrote its position 0.
#   It is recomputed whenever a slot is prefilled from position 0 (a new call, a session admission), never by decode passes or later
#   prefill passes of the same sequence.
# Call kinds.  Best-of-N siblings get the source slot's centre with its rows.  With a shared text prefix every sequence of the call
#   takes sequence 0's centre, which exists before any row of the call is packed.
# K codes and shifts: the kv8 grid applied to bf16_rne(float(k) - float(c)).  V is plain kv8.
# Scores: a position read from the 8-bit cache scores (q . k8) * 2**s + q . c; the pass's own positions come from the bf16 cache, uncentred.
def kv8c_centre(k_rows: torch.Tensor) -> torch.Tensor:
    """bf16-valued K rows [..., n0, hd] of one head -> their centre [..., hd]: the fp32 mean, rounded to bf16 (returned as fp32)."""
    return k_rows.detach().to(torch.float32).mean(dim=-2).bfloat16().float()


def _kv8c_centred(k: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    k, c = k.detach().to(torch.float32), c.detach().to(torch.float32)
    assert bool((c == c.bfloat16().float()).all()), "a bf16 centre"
    return (k - c.unsqueeze(-2)).bfloat16().float()


def kv8c_quantize_rows(k: torch.Tensor, c: torch.Tensor):
    """K rows [..., n, hd] against their head's centre c [..., hd] -> (codes, shift) of bf16_rne(k - c) on the kv8 grid: what the centred
    packer must match bit for bit."""
    return kv8_quantize_rows(_kv8c_centred(k, c))


def kv8c_roundtrip(k: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """What the 8-bit cache of a centred engine holds for the rows k: the grid's value of k - c.  The attention's scores are those of
    c + kv8c_roundtrip(k, c)."""
    return kv8_roundtrip(_kv8c_centred(k, c))
