"""tests/prefill_attn_cases.py without a GPU: every launch obeys the layout rule of a prefill pass; the q handed to the kernels rounds
back to the bf16-exact log2-unit vector the reference uses; the restated key partition covers [0, last] exactly once for every row
tile; the float64 reference agrees with torch's scaled_dot_product_attention in float64; the inputs are what the families promise;
and every launch is ADMITTED - each defect model moves some element by at least 8 bars at every covered position, so a kernel inside
its bar has not lost, doubled, misplaced or leaked a covered position."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import decode_attn_cases as dc
import prefill_attn_cases as pc

FORM_IDS = [f"f{form}-{dtype}-hd{hd}" for form, dtype, hd in pc.FORMS]


@functools.lru_cache(maxsize=2)
def _launches(form, dtype, hd):
    return pc.all_launches(form, dtype, hd)


def test_geometry_matches_the_issue():
    assert len(pc.FORMS) == 7 and pc.FORMS[-1] == (2, "bf16", 128)
    assert [pc.kw(*f[:2]) for f in pc.FORMS] == [16, 16, 16, 32, 32, 32, 64] and pc.NW * pc.kw(1, "bf16") == 128 and pc.NW * pc.kw(1, "fp32") == 64
    assert pc.sweep_rows(1) == 320 > 2 * 128 and pc.sweep_rows(2) == 384 > 5 * 64          # a second visit of every wave; both LDS stages twice
    assert [s for s, _ in pc.share_values(1, "bf16")] == [1, 31, 32, 33, 127, 129, 53, 190]
    assert [s for s, _ in pc.share_values(1, "fp32")] == [1, 15, 16, 17, 63, 65, 85, 94]
    assert [s for s, _ in pc.share_values(2, "bf16")] == [1, 62, 63, 64, 65, 127, 128, 129, 165]
    for form, dtype, _ in pc.FORMS:          # a share whose row tiles start one position in front of a key tile's last key; one inside the last key tile
        KW, vals = pc.kw(form, dtype), pc.share_values(form, dtype)
        assert any(s % KW == KW - 2 for s, _ in vals) and (form == 2 or any((s + t - 1) // KW == s // KW and t <= 3 for s, t in vals))
    assert sorted((n - 1) % 16 + 1 for n, _ in pc.RAGGED[1])[:1] == [1] and {15, 16} <= {(n - 1) % 16 + 1 for n, _ in pc.RAGGED[1]}
    assert [(n - 1) % 64 + 1 for n, _ in pc.RAGGED[2]] == [1, 16, 17, 63, 64]
    assert min(n for n, _ in pc.RAGGED[1]) < pc.kw(1, "fp32")                                # waves without a key tile join the merge
    assert [p0 for _, p0 in pc.CONT[1]] == [16, 128, 144] and [p0 for _, p0 in pc.CONT[2]] == [64, 192]
    assert pc.SENS_MIN == 8.0 and pc.BAR32 == 2.0 ** -18 and pc.BAR16_P == 2.0 ** -7 and pc.BAR16_OUT == 2.0 ** -8


@pytest.mark.parametrize("form,dtype,hd", pc.FORMS, ids=FORM_IDS)
def test_every_launch_obeys_the_layout_and_the_q_round_trip(form, dtype, hd):
    """check_layout on every launch; numpy float32 q * (float32 scale * float32 log2 e) rounds to the bf16-exact qhat for every q."""
    kinds = set()
    c = np.float32(dc.kernel_scale(hd)) * np.float32(1.4426950408889634)
    assert c.dtype == np.float32 and float(c) == pc.qs(hd)
    for L in _launches(form, dtype, hd):
        pc.check_layout(L)
        kinds.add((L.kind, L.family))
        assert np.array_equal(L.qhat, dc.bf16_exact(L.qhat)) and L.q.dtype == np.float32
        back = L.q * c
        assert back.dtype == np.float32 and np.array_equal(dc.bf16_exact(back), L.qhat), L.name
        for a in (L.Kf, L.Vf):
            assert np.array_equal(a, dc.bf16_exact(a)), L.name
        assert len(L.prompts) >= 3 or L.kind == "sweep" or (L.kind == "cont" and form == 2)
    assert {k for k, _ in kinds} == {"sweep", "ragged", "short", "cont", "share"}
    assert {f for _, f in kinds} == {"flat", "uniform", "probe", "peaked"}
    assert (("sweep", "flat") in kinds) == (dtype == "fp32")          # flat is listed for the bf16 forms only where it separates a position


@pytest.mark.parametrize("form,dtype,hd", pc.FORMS, ids=FORM_IDS)
def test_the_key_partition_covers_every_row_tile_once(form, dtype, hd):
    """Every workgroup of every launch: the key tiles its waves visit, each cut at the last key the kernel clamps to, cover [0, last]
    exactly once (form 2: per wave, [0, last position of the wave's rows]); a tile never starts behind `last`."""
    KW, al = pc.kw(form, dtype), pc.align(form)
    idle = 0
    for L in _launches(form, dtype, hd):
        for r0 in range(0, L.rows, al):
            rp = L.row_pos[r0:r0 + al]
            na = int((rp >= 0).sum())
            if na == 0:
                continue
            assert (rp[:na] == rp[0] + np.arange(na)).all() and len(set(L.row_seq[r0:r0 + na])) == 1
            last = int(rp[0]) + na - 1
            if form == 1:
                seen = np.zeros(last + 1, dtype=int)
                for w in range(pc.NW):
                    tiles, lim = pc.key_tiles(form, dtype, int(rp[0]), na, w)
                    idle += not tiles
                    for kt0 in tiles:
                        assert kt0 <= lim == last
                        seen[kt0:min(kt0 + KW, last + 1)] += 1
                assert (seen == 1).all()
            else:
                for w in range(4):
                    tiles, t_last = pc.key_tiles(form, dtype, int(rp[0]), na, w)
                    if na <= 16 * w:
                        idle += 1
                        assert not tiles
                        continue
                    seen = np.zeros(t_last + 1, dtype=int)
                    for kt0 in tiles:
                        seen[kt0:min(kt0 + KW, t_last + 1)] += 1
                    assert (seen == 1).all() and tiles == list(range(0, t_last + 1, KW)) and t_last <= last
    assert idle > 0          # waves without a key tile (form 2: without an active row) are among the cases


@pytest.mark.parametrize("form,dtype,hd", [(1, "fp32", 32), (1, "bf16", 64), (2, "bf16", 128)])
def test_reference_against_sdpa(form, dtype, hd):
    """One launch per layout kind and family: the reference against F.scaled_dot_product_attention in float64 (softmax2(x) is
    softmax(x ln 2)), with and without foreign data below the prefix; padding rows are zeros."""
    done = set()
    for L in _launches(form, dtype, hd):
        if (L.kind, L.family) in done:
            continue
        done.add((L.kind, L.family))
        for own in (False, True) if L.share else (False,):
            K, V = pc.kernel_caches(L, own_prefix=own)
            ref, b32, b16 = pc.reference(L, K, V)
            active = L.row_pos >= 0
            assert np.isfinite(ref).all() and (ref[~active] == 0).all() and (b32[active] > 0).all() and (b16[active] >= b32[active]).all()
            for s, p0, n, r0 in L.prompts:
                sh = min(L.share, p0 + n) if s else 0
                Kr = torch.from_numpy(np.concatenate([K[0, :, :sh], K[s, :, sh:p0 + n]], axis=1)).double()
                Vr = torch.from_numpy(np.concatenate([V[0, :, :sh], V[s, :, sh:p0 + n]], axis=1)).double()
                assert torch.isfinite(Kr).all() and torch.isfinite(Vr).all()
                qh = torch.from_numpy(L.qhat[r0:r0 + n].reshape(n, pc.H, hd)).double().transpose(0, 1)
                vis = torch.arange(p0 + n)[None, :] <= (p0 + torch.arange(n))[:, None]
                want = F.scaled_dot_product_attention(qh, Kr, Vr, attn_mask=vis, scale=float(np.log(2.0)))
                want = want.transpose(0, 1).reshape(n, -1).numpy()
                assert np.abs(ref[r0:r0 + n] - want).max() <= 1e-12 * float(Vr.abs().max()), L.name
    assert len(done) >= 14


@pytest.mark.parametrize("form,dtype,hd", pc.FORMS, ids=FORM_IDS)
def test_inputs_are_what_the_families_promise(form, dtype, hd):
    KW = pc.kw(form, dtype)
    residues, edges, crossed = set(), set(), 0
    for L in _launches(form, dtype, hd):
        K, V = pc.kernel_caches(L)
        used = {s for s, _, _, _ in L.prompts}
        for s in range(L.n_slots):
            if s not in used:
                assert np.isnan(K[s]).all() and np.isnan(V[s]).all()          # the unused slot
        for pi, (s, p0, n, r0) in enumerate(L.prompts):
            last = p0 + n - 1
            assert np.isnan(K[s, :, last + 1:]).all() and np.isnan(V[s, :, last + 1:]).all()
            lo = L.share if s else 0
            assert np.isnan(K[s, :, :lo]).all() and np.isfinite(K[s, :, lo:last + 1]).all() and np.isfinite(V[s, :, lo:last + 1]).all()
            Ko, Vo = pc.kernel_caches(L, own_prefix=True)
            assert np.isfinite(Ko[s, :, :last + 1]).all() and (lo == 0 or not np.array_equal(Vo[s, :, :lo], Vo[0, :, :lo]))
            ev = pc.prompt_eval(L, K, V, pi)
            sc = np.where(ev["vis"][None], np.einsum("nhd,hsd->hns", ev["qh"], ev["Kr"]), np.nan)
            w = ev["e"] / ev["D"][..., None]
            if L.family == "flat":
                assert np.nanmax(np.abs(sc)) <= 0.25 and 0.5 <= np.abs(ev["Vr"]).min() and np.abs(ev["Vr"]).max() <= 1.5
            elif L.family == "uniform":
                assert (np.nanmax(sc, axis=-1) == np.nanmin(sc, axis=-1)).all()          # one number per row, in float64 as anywhere
                assert (ev["e"][:, ev["vis"]] == 1).all() and np.array_equal(ev["Vr"], np.round(ev["Vr"])) and np.abs(ev["Vr"]).max() <= 128
            elif L.family == "probe":
                P = L.covered[s]
                assert len(P) <= pc.N_PROBES and len(P) == len(set(P)) and {0, last} <= set(P) and (not L.share or {L.share - 1, L.share} & set(P))
                assert p0 in P or p0 > last
                for p in P:
                    assert abs(sc[:, max(p - p0, 0), p] - pc.LIFT2).max() < 0.15
                    if p >= max(p0, 1):
                        residues.add(p % KW)
                        edges |= {p % KW} & {0, KW - 1}
                rest = np.setdiff1d(np.arange(last + 1), P)
                if len(rest):
                    assert np.nanmax(np.abs(sc[:, :, rest])) <= 0.25
                assert w[:, -1, P].min() >= 0.035, (L.name, w[:, -1, P].min())          # each probe holds a few per cent of the longest row
            else:
                P = L.covered[s]
                run = sc[:, -1, P]
                assert (run == run[:, :1]).all() and (run == np.nanmax(sc[:, -1], axis=-1, keepdims=True)).all() and run.min() > 127
                crossable = any(b - 2 >= p0 and b + 2 <= last for b in range(KW, last + 1, KW))
                R = P if last < pc.RUN else P[1:]          # position 0 holds the maximum too; the run lies behind it
                assert P[0] == 0 and len(R) == min(pc.RUN, last + 1) and (R == R[0] + np.arange(len(R))).all()
                assert not crossable or (R[0] >= max(p0, 1) and R[0] // KW != R[-1] // KW)
                assert (np.nanmax(sc, axis=-1) == run[:, :1]).all()          # every row's largest score is that maximum
                crossed += crossable
                assert np.nanmin(sc) < -127 or last < 64
    assert residues == set(range(KW)), sorted(set(range(KW)) - residues)          # the lifted diagonals take every residue modulo KW
    assert edges == {0, KW - 1} and crossed >= 3          # peaked runs across a key-tile boundary, rows inside the run


@pytest.mark.parametrize("form,dtype,hd", pc.FORMS, ids=FORM_IDS)
def test_every_launch_is_admitted(form, dtype, hd):
    low = {}
    for L in _launches(form, dtype, hd):
        assert L.family in pc.families(form, dtype, L.kind)
        res = pc.launch_sensitivity(L)
        need = {"drop", "twice", "neighbour", "beyond"} | ({"own_prefix"} if L.share else set())
        assert need <= set(res), (L.name, sorted(res))
        assert min(res.values()) >= pc.SENS_MIN, (L.name, res)
        low[L.family] = min(low.get(L.family, np.inf), min(res.values()))
    print(f"form {form} {dtype} hd {hd}: smallest defect / bar per family {({k: round(v, 1) for k, v in low.items()})}")


def test_flat_is_not_admitted_for_bf16_beyond_short_prompts():
    """Why the bf16 forms do not list the flat family in the sweep: one flat position in a few hundred is below 8 bars."""
    L = pc.make_launch(1, "bf16", 32, "flat", "sweep", [(320, 0)])
    assert min(pc.launch_sensitivity(L).values()) < pc.SENS_MIN
