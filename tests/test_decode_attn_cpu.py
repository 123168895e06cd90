"""tests/decode_attn_cases.py without a GPU: the restated chunk rule partitions every row; the float64 reference and the merge agree
with torch's scaled_dot_product_attention in float64 under any partition; the inputs are what the families promise; and every case
of the table is ADMITTED - each defect model moves some element of the merged reference row by at least 8 times that element's bar,
so a kernel inside its bar has not lost, doubled or misplaced a covered position."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decode_attn_cases as dc


def test_the_chunk_rule_partitions_every_row():
    S = np.arange(1, 8193)
    over = 0
    for n in range(1, dc.MAX_NSPLIT + 1):
        c = dc.chunk_rule(S, n)
        assert (c >= 1).all() and (c * n >= S).all(), n              # the chunks [i c, min(S, (i + 1) c)) cover [0, S) ...
        ceil = (S + n - 1) // n
        assert (c >= ceil).all()
        over += int((c > ceil).sum())
        assert (c <= ceil + 1).all(), n                              # ... and a chunk is never more than one too long
    print(f"chunk one above ceil(S / n) at {over} of {8 * len(S)} (S, n)")
    for S_, n in ((1, 8), (9, 8), (8192, 7), (4161, 3), (577, 5)):    # the pieces themselves, spelled out
        cuts = dc.splits(S_, n)
        seen = np.zeros(S_, dtype=int)
        for p0, p1 in cuts:
            seen[p0:p1] += 1
        assert (seen == 1).all() and len(cuts) == n
    assert dc.empty_last_split(8) == 9 and dc.splits(9, 8)[-1][0] >= 9
    assert [dc.empty_last_split(n) for n in (1, 2)] == [None, None]


def test_geometry_matches_the_issue():
    assert [dc.ppw("bf16", hd) for hd in dc.HDS] == [16, 8, 4] and [dc.ppw("fp32", hd) for hd in dc.HDS] == [8, 4, 2]
    assert dc.sweep_top("bf16", 32) == 4161 and dc.sweep_top("fp32", 128) == 577
    for dtype in dc.DTYPES:
        for hd in dc.HDS:
            for n in dc.EDGE_NSPLITS:
                P, B, ls = dc.ppw(dtype, hd), dc.batch(dtype, hd), set(dc.edge_lengths(dtype, hd, n))
                want = {1, 2, n, n + 1, P - 1, P + 1, 8 * P - 1, 8 * P + 1, B - 1, B, B + 1, n * B - 1, n * B, n * B + 1, 2 * B + 1}
                assert want <= ls and (n == 1 or n - 1 in ls) and max(ls) == max(n * B + 1, 2 * B + 1)
                assert n <= 2 or any(dc.splits(S, n)[-1][0] >= S for S in ls if S > n)
                assert n == 1 or any(S < n for S in ls)              # most splits empty


@pytest.mark.parametrize("hd", dc.HDS)
def test_reference_and_merge_against_sdpa(hd):
    """The per-row reference, the prefix-sum reference of the sweep and merge(split_partials) under the kernel's partition and under
    arbitrary ones, all against F.scaled_dot_product_attention in float64."""
    rng = np.random.RandomState(hd)
    for family, share in (("flat", 0), ("probe", 0), ("peaked", 0), ("flat", 37), ("probe", 37)):
        L = dc.make_launch("bf16", hd, 5, family, (1, 2, 36, 37, 38, 150, 301, 300), share=share)
        K, V = dc.kernel_caches(L)
        ref, b32, b16 = dc.reference(L, K, V)
        assert np.isfinite(ref).all() and (b16 > b32).all() and (b32 > 0).all()
        for i in range(L.rows):
            Kr, Vr = dc.row_kv(L, K, V, i)
            assert np.isfinite(Kr).all() and np.isfinite(Vr).all()
            qr = torch.from_numpy(L.q[i].reshape(dc.H, 1, hd)).double()
            want = F.scaled_dot_product_attention(qr, torch.from_numpy(Kr), torch.from_numpy(Vr), scale=dc.kernel_scale(hd))
            want = want.reshape(-1).numpy()
            assert np.abs(ref[i] - want).max() <= 1e-13 * np.abs(Vr).max()
            S = Kr.shape[1]
            edges = np.sort(rng.randint(0, S + 1, size=6))
            for cuts in (dc.splits(S, 5), dc.splits(S, 8), list(zip(np.r_[0, edges], np.r_[edges, S]))):
                O, ML = dc.split_partials(L.q[i].reshape(dc.H, hd), Kr, Vr, hd, cuts)
                ML[:, [j for j, (p0, p1) in enumerate(cuts) if p0 >= p1], 0] = 1e30      # an empty partial's maximum is not read
                got = dc.merge(O[None], ML[None])[0]
                assert np.abs(got - want).max() <= 1e-13 * np.abs(Vr).max()
        assert np.abs(dc.restate_fp32(L, K, V) - ref).max() <= dc.BAR32 * 1.5            # fp32 alone stays far inside the bar
    # a row without a live partial is NaN, never a number
    assert np.isnan(dc.merge(np.zeros((1, dc.H, 3, hd)), np.tile([-np.inf, 0.0], (1, dc.H, 3, 1)))).all()
    # the sweep's prefix sums
    out, bar = dc.sweep_reference("fp32", hd)
    lengths = (1, 2, 63, 64, 65, dc.sweep_top("fp32", hd))
    L = dc.sweep_launch("fp32", hd, lengths)
    ref, b32, _ = dc.reference(L)
    for i, S in enumerate(lengths):
        c = 0 if L.row_seq[i] == 0 else 1
        assert np.abs(out[c, (S - 1) % dc.NQ, S - 1] - ref[i]).max() <= 1e-12
        assert np.array_equal(np.repeat(bar[c, S - 1], hd), b32[i])


def test_inputs_are_what_the_families_promise():
    for dtype, hd in (("bf16", 32), ("fp32", 128)):
        for family in ("flat", "probe", "peaked"):
            L = dc.make_launch(dtype, hd, 8, family, dc.edge_lengths(dtype, hd, 8))
            K, V = dc.kernel_caches(L)
            assert sorted(L.row_seq) == list(range(L.rows)) and (L.row_seq != np.arange(L.rows)).all()
            for a in (L.q, L.Kf, L.Vf):
                assert np.array_equal(a, dc.bf16_exact(a))                        # both dtypes read the same numbers
            aV = np.abs(L.Vf)
            assert aV.min() >= 0.5 and aV.max() <= 1.5 and (L.Vf < 0).any() and (L.Vf > 0).any()
            for i in range(L.rows):
                s, pos = L.row_seq[i], L.row_pos[i]
                assert np.isnan(K[s, :, pos + 1:]).all() and np.isnan(V[s, :, pos + 1:]).all()
                Kr, Vr = dc.row_kv(L, K, V, i)
                ev = dc.row_eval(L.q[i].reshape(dc.H, hd), Kr, Vr, hd)
                w = ev["e"] / ev["D"][:, None]
                P = L.covered[i]
                if family == "flat":
                    assert np.abs(ev["sc"]).max() <= 0.25 and w.max() / w.min() <= np.exp(0.5) + 1e-9
                elif family == "probe":
                    assert len(P) == min(dc.N_PROBES, pos + 1) and {0, pos} <= set(P)
                    assert np.abs(ev["sc"][:, P] - dc.LIFT).max() < 0.1
                    assert w[:, P].min() >= 0.035, (pos, w[:, P].min())           # each probe holds a few per cent of the row
                    for p0, p1 in dc.splits(pos + 1, 8):                          # chunk ends are probed wherever 16 probes reach
                        if pos + 1 <= 64 and p0 < p1:
                            assert pos + 1 <= dc.N_PROBES or {p0, p1 - 1} & set(P)
                else:
                    assert ev["sc"].max() > 88 and (pos < 64 or ev["sc"].min() < -88)
                    run = ev["sc"][:, P]
                    assert (run == run[:, :1]).all() and (run == ev["sc"].max(axis=1, keepdims=True)).all()
                    assert len(P) == min(dc.RUN, pos + 1)
    # shared prefix: the other sequences hold NaN below it, and rows on both sides of it are in the launch
    L = dc.share_launch("bf16", 64, 4, dc.batch("bf16", 64) + 3, "probe")
    K, V = dc.kernel_caches(L)
    assert L.row_seq[-1] == 0 and L.row_pos[-1] + 1 >= L.share
    assert np.isnan(K[1:, :, : L.share]).all() and np.isfinite(K[0, :, : L.share]).all()
    assert (L.row_pos + 1 < L.share).any() and (L.row_pos + 1 == L.share).any() and (L.row_pos + 1 > L.share + dc.batch("bf16", 64)).any()


def _admit(L, out_kinds):
    res = dc.launch_sensitivity(L)
    need = {"twice", "beyond", "drop", "neighbour"} | ({"own_prefix"} if L.share else set())
    assert need <= set(res), (L.name, sorted(res))
    worst = {k: min(v[0 if kind == "fp32" else 1] for kind in out_kinds) for k, v in res.items()}
    assert min(worst.values()) >= dc.SENS_MIN, (L.name, out_kinds, worst)
    return min(worst.values())


@pytest.mark.parametrize("hd", dc.HDS)
@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_every_edge_case_is_admitted(dtype, hd):
    low = {}
    for n in dc.EDGE_NSPLITS:
        for family, L in dc.edge_launches(dtype, hd, n).items():
            kinds = ("fp32",) if family == "flat" else ("fp32", "bf16")
            low[family] = min(low.get(family, np.inf), _admit(L, kinds))
    print(f"{dtype} hd {hd}: smallest defect / bar per family {({k: round(v, 1) for k, v in low.items()})}")


@pytest.mark.parametrize("hd", dc.HDS)
@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_every_shared_prefix_case_is_admitted(dtype, hd):
    low = {}
    for n in dc.SHARE_NSPLITS:
        for share in dc.share_values(dtype, hd):
            for family in ("flat", "probe"):
                L = dc.share_launch(dtype, hd, n, share, family)
                low[family] = min(low.get(family, np.inf), _admit(L, ("fp32",) if family == "flat" else ("fp32", "bf16")))
    print(f"{dtype} hd {hd}: smallest defect / bar per family {({k: round(v, 1) for k, v in low.items()})}")


@pytest.mark.parametrize("hd", dc.HDS)
@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_the_sweep_is_admitted_at_every_length(dtype, hd):
    """Flat rows against the fp32-output bar, every S = 1 .. sweep_top: the defect / bar ratio falls with S, so the 64 longest rows, every
    64th below them and the shortest ones are computed."""
    top = dc.sweep_top(dtype, hd)
    lengths = sorted(set(range(1, 18)) | set(range(64, top - 64, 64)) | set(range(top - 63, top + 1)))
    low = np.inf
    for i in range(0, len(lengths), 32):
        part = lengths[i:i + 32]
        if len(part) < 2:
            part = lengths[i - 1:i + 32]
        res = dc.launch_sensitivity(dc.sweep_launch(dtype, hd, part))
        low = min(low, min(v[0] for v in res.values()))
    print(f"{dtype} hd {hd}: smallest defect / fp32 bar over S = 1..{top}: {low:.1f}")
    assert low >= dc.SENS_MIN
