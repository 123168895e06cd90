"""tile_attn_k (fp32 / bf16 x head_dim 32 / 64 / 128) and tile_attn64_k against float64, position by position
(tests/prefill_attn_cases.py holds the launches, the reference, the bars and the proof that a kernel inside its bar has not lost,
doubled, misplaced or leaked a covered position; tests/test_prefill_attn_cpu.py runs it).

A kernel is launched through vc_debug_tile_attn on buffers of the test: H = 2 heads, a prefill pass's row stream of at most 704 rows,
every position a row must not read NaN, x_out preset to a sentinel with guard rows behind it.  Every element of every active row is
judged against
    fp32 forms   2^-18 max|V|        bf16 forms   that + 2^-7 sum_p w_p |V_pj|   (uniform family: that + 2^-8 |ref_j|)
padding rows must hold exact zeros and the guard rows their sentinel.  Each test asserts the census slot its launches counted in and
prints the largest fraction of the bar the kernel used per family."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import prefill_attn_cases as pc

pytestmark = pytest.mark.gpu

SENT = 16384.0          # preset of x_out (exact in bf16): an unwritten element shows
GUARD = 16              # rows behind the launch's that must keep the preset
DEV = "cuda:0"
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
FORM_IDS = [f"f{form}-{dtype}-hd{hd}" for form, dtype, hd in pc.FORMS]
assert len(pc.FORMS) == 7          # the compiled forms of tile_attn_k and tile_attn64_k


@pytest.fixture(scope="module")
def census():
    """The process-wide launch census, read through a tiny engine (the kernels under test need none)."""
    from voicecraft_amd import synth
    from voicecraft_amd.engine import VoiceCraftEngine
    a = synth.make_args("tiny")
    eng = VoiceCraftEngine(a, synth.make_state_dict(a, seed=1), device=DEV, dtype="bf16", max_seqs=1, max_positions=256)
    return eng.launch_counts


class _Counted:
    """Asserts on exit that exactly the launches made inside went through the form's launcher."""

    def __init__(self, census, form):
        self.census, self.form, self.n = census, form, 0

    def __enter__(self):
        self.c0 = self.census()
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            c = self.census()
            d = {k: c[k] - self.c0[k] for k in ("tile_attn", "tile_attn64", "rows_attn")}
            assert self.n > 0 and d == {"tile_attn": self.n, "tile_attn64": self.n if self.form == 2 else 0, "rows_attn": 0}, (d, self.n)


def _i32(x):
    return torch.tensor(np.asarray(x, dtype=np.int32).reshape(-1), dtype=torch.int32, device=DEV)


def _device_entry(L):
    t = TDT[L.dtype]
    K, V = pc.kernel_caches(L)
    ref, b32, b16 = pc.reference(L, K, V)
    e = dict(L=L, name=L.name, family=L.family, form=L.form, q=torch.from_numpy(L.q).to(DEV), row_seq=_i32(L.row_seq), row_pos=_i32(L.row_pos),
             share=_i32([L.share]), K=torch.from_numpy(K).to(DEV).to(t), V=torch.from_numpy(V).to(DEV).to(t), ref=ref,
             bar=b32 if L.dtype == "fp32" else b16, active=L.row_pos >= 0)
    if L.share:          # the second variant: foreign finite data below the prefix in the other sequences' own slots (same reference)
        Ko, Vo = pc.kernel_caches(L, own_prefix=True)
        e["Ko"], e["Vo"] = torch.from_numpy(Ko).to(DEV).to(t), torch.from_numpy(Vo).to(DEV).to(t)
    return e


def _used(e, own=False):
    """One launch of the entry; the largest |got - ref| / bar over its active rows (a NaN or an infinity counts as infinitely far)."""
    from voicecraft_amd import engine
    x = engine.debug_tile_attn(e["q"], e["Ko" if own else "K"], e["Vo" if own else "V"], e["row_seq"], e["row_pos"], e["share"], form=e["form"],
                               sentinel=SENT, guard_rows=GUARD).double().cpu().numpy()
    rows = len(e["active"])
    assert (x[rows:] == SENT).all(), (e["name"], "the launch wrote behind its rows")
    x = x[:rows]
    assert not (x == SENT).any(), (e["name"], "x_out elements left unwritten")
    assert (x[~e["active"]] == 0).all(), (e["name"], "a padding row is not exact zeros")
    act = e["active"]
    f = np.where(np.isfinite(x[act]), np.abs(x[act] - e["ref"][act]) / e["bar"][act], np.inf)
    return float(f.max())


def _sweep(entries, census, form, what):
    worst = {}
    with _Counted(census, form) as cnt:
        for e in entries:
            for own in (False, True) if "Ko" in e else (False,):
                u = _used(e, own)
                cnt.n += 1
                worst[e["family"]] = max(worst.get(e["family"], 0.0), u)
                assert u <= 1.0, (e["name"], "own_prefix" if own else "", u)
    print(f"\n{what}: fraction of the bar used per family {({k: round(v, 3) for k, v in worst.items()})}")
    return worst


@functools.lru_cache(maxsize=1)
def _entries(kind, form, dtype, hd):
    return [_device_entry(L) for L in getattr(pc, kind + "_launches")(form, dtype, hd)]


@pytest.mark.parametrize("form,dtype,hd", pc.FORMS, ids=FORM_IDS)
def test_every_length_at_once(census, form, dtype, hd):
    """One sequence of 320 rows (tile_attn64_k: 384) from position 0: every S = 1..rows in one launch - a second visit of every wave of
    tile_attn_k (NW KW = 128 keys in bf16, 64 in fp32), both LDS stages of tile_attn64_k twice - in every family listed for the form;
    the probe variants' lifted diagonals take every residue modulo the key-tile width."""
    es = _entries("sweep", form, dtype, hd)
    assert {e["family"] for e in es} == set(pc.families(form, dtype, "sweep")) and all(e["L"].rows == pc.sweep_rows(form) for e in es)
    _sweep(es, census, form, f"form {form} {dtype} hd {hd}, every S = 1..{pc.sweep_rows(form)}")


@pytest.mark.parametrize("form,dtype,hd", pc.FORMS, ids=FORM_IDS)
def test_ragged_streams(census, form, dtype, hd):
    """Five prompts side by side (blocks of different sequences adjacent): last tiles of 1, 15 and 16 rows, a prompt shorter than one key
    tile (waves without a key tile join the merge); tile_attn64_k: last blocks of 1, 16, 17, 63 and 64 rows (waves without an active
    row).  And the `short` stream, every prompt inside one 16-row tile, where the flat family still separates a position in bf16."""
    es = _entries("ragged", form, dtype, hd)
    assert {e["L"].kind for e in es} == {"ragged", "short"} and all(len(e["L"].prompts) >= 3 for e in es)
    _sweep(es, census, form, f"form {form} {dtype} hd {hd}, ragged streams")


@pytest.mark.parametrize("form,dtype,hd", pc.FORMS, ids=FORM_IDS)
def test_continuation_passes(census, form, dtype, hd):
    """p0 = 16, 128 and 144 (tile_attn64_k: 64 and 192): the earlier positions are present only in the cache."""
    es = _entries("cont", form, dtype, hd)
    assert all(sorted(p[1] for p in e["L"].prompts) == sorted(p0 for _, p0 in pc.CONT[form]) for e in es)
    _sweep(es, census, form, f"form {form} {dtype} hd {hd}, continuation passes")


@pytest.mark.parametrize("form,dtype,hd", pc.FORMS, ids=FORM_IDS)
def test_shared_prefix(census, form, dtype, hd):
    """share = 1, KW - 1, KW, KW + 1, NW KW +- 1, 16 k + 5 and a value inside the last key tile (tile_attn64_k: 1, 63, 64, 65, 127..129,
    64 k + 37, 62): sequence 0 holds the prefix rows, two others start at p0 = share, so their row tiles sit at unaligned positions and the
    prefix boundary falls inside a key tile.  Each launch twice: NaN below the prefix in the other sequences' own slots, then foreign
    finite numbers there."""
    es = _entries("share", form, dtype, hd)
    assert [e["L"].share for e in es if e["family"] == "uniform"] == [s for s, _ in pc.share_values(form, dtype)]
    assert all("Ko" in e and any(p[0] == 0 for p in e["L"].prompts) and sum(p[1] == e["L"].share for p in e["L"].prompts) == 2 for e in es)
    _sweep(es, census, form, f"form {form} {dtype} hd {hd}, shared prefix")


@pytest.mark.parametrize("form,dtype,hd", pc.FORMS, ids=FORM_IDS)
def test_rows_that_must_leave_nothing(census, form, dtype, hd):
    """A launch of padding only (row_pos = -1 everywhere, the caches NaN throughout): exact zeros in its rows, the guard rows keep the
    sentinel."""
    from voicecraft_amd import engine
    rows, t = 2 * pc.align(form), TDT[dtype]
    q = torch.from_numpy(pc.content(hd, 8)[0][np.arange(rows) % 4].reshape(rows, -1).copy()).to(DEV)
    K = torch.full((2, pc.H, 48, hd), float("nan"), dtype=t, device=DEV)
    with _Counted(census, form) as cnt:
        x = engine.debug_tile_attn(q, K, K.clone(), _i32(np.zeros(rows)), _i32(np.full(rows, -1)), _i32([0]), form=form, sentinel=SENT,
                                   guard_rows=GUARD)
        cnt.n += 1
    x = x.double().cpu().numpy()
    assert (x[:rows] == 0).all() and (x[rows:] == SENT).all() and x.shape[0] == rows + GUARD


def test_refusals_with_real_buffers(census):
    """What no prefill pass can issue is refused (VC_EINVAL) before anything is launched: x_out keeps its preset, the census stands."""
    from voicecraft_amd import _lib
    lib = _lib.load()
    hd, S_max, rows = 128, 96, 64
    q = torch.zeros((rows, pc.H * hd), device=DEV)
    kc = torch.zeros((2, pc.H, S_max, hd), dtype=torch.bfloat16, device=DEV)
    vc = torch.zeros_like(kc)
    x = torch.full((rows, pc.H * hd), SENT, dtype=torch.bfloat16, device=DEV)
    seq, pos, zero = _i32(np.ones(rows)), _i32(np.arange(rows)), _i32([0])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        base = dict(q=q.data_ptr(), kcache=kc.data_ptr(), vcache=vc.data_ptr(), row_seq=seq.data_ptr(), row_pos=pos.data_ptr(),
                    share_len=zero.data_ptr(), x_out=x.data_ptr(), dtype=1, H=pc.H, hd=hd, S_max=S_max, rows=rows, form=1)
        base.update(kw)
        return lib.vc_debug_tile_attn(C.byref(_lib.DebugTileAttnArgs(**base)), stream)

    c0 = census()
    for kw in (dict(hd=48), dict(hd=16), dict(hd=256), dict(form=0), dict(form=3), dict(form=2, dtype=0), dict(form=2, hd=64), dict(rows=0),
               dict(rows=-16), dict(rows=24), dict(rows=63), dict(form=2, rows=48), dict(form=2, rows=32), dict(H=0), dict(S_max=0), dict(dtype=2),
               dict(q=None), dict(kcache=None), dict(vcache=None), dict(row_seq=None), dict(row_pos=None), dict(share_len=None), dict(x_out=None),
               dict(q=q.data_ptr() + 4), dict(kcache=kc.data_ptr() + 8), dict(vcache=vc.data_ptr() + 2), dict(x_out=x.data_ptr() + 8)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (x == SENT).all() and census() == c0
    assert call() == 0 and call(form=2) == 0 and call(rows=48) == 0 and call(rows=16) == 0          # and the legal neighbours run
    torch.cuda.synchronize()
    assert not (x == SENT).any()
    c = census()
    assert c["tile_attn"] - c0["tile_attn"] == 4 and c["tile_attn64"] - c0["tile_attn64"] == 1
