"""The C-ABI boundary without a GPU: the shared library loads, exports every symbol that
include/*.h declares with the declared arity, and refuses loudly to run when there is no device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    out = {}
    inc = os.path.join(ROOT, "include")
    for fn in sorted(os.listdir(inc)):
        src = open(os.path.join(inc, fn)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        for m in re.finditer(r"\b(?:int|void|const char\s*\*)\s*(vc_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
            args = m.group(2).strip()
            n = 0 if args in ("", "void") else args.count(",") + 1
            out[m.group(1)] = n
    return out


@pytest.fixture(scope="module")
def lib():
    from voicecraft_amd import _lib
    return _lib.load()


def test_every_declared_symbol_is_exported_and_bound(lib):
    from voicecraft_amd import _lib, codec
    decl = _declared()
    assert len(decl) >= 15
    protos = dict(_lib.PROTOTYPES)
    protos.update(codec.PROTOTYPES)
    for name, nargs in decl.items():
        assert hasattr(lib, name), f"{name} declared in include/ but not exported by libvcengine.so"
        assert name in protos, f"{name} has no ctypes prototype"
        assert len(protos[name][1]) == nargs, f"{name}: header has {nargs} parameters, binding has {len(protos[name][1])}"
    for name in protos:
        assert name in decl, f"{name} bound in Python but not declared in include/"


def test_build_refuses_a_listed_source_that_is_missing(monkeypatch):
    """A unit listed in build.SOURCES but absent from csrc/ is an error that names the file: the -shared link accepts undefined
    symbols, so the library would build without the unit and fail only when it is loaded."""
    from voicecraft_amd import build
    monkeypatch.setattr(build, "SOURCES", build.SOURCES + ["vc_engine_misspelt.hip"])
    with pytest.raises(FileNotFoundError, match="vc_engine_misspelt.hip"):
        build.build()


def test_struct_layout_matches_header():
    from voicecraft_amd._lib import ModelCfg, SampleCfg
    assert C.sizeof(ModelCfg) == 17 * 4
    # int32 top_k, float top_p, float temperature, int32 stop_repetition, int32 n_silence, int32[8], (pad) u64 seed,
    # 3x int32 (use_graph, poll_every, forced_mode) + tail padding to the 8-byte alignment of the struct
    assert SampleCfg.seed.offset % 8 == 0 and C.sizeof(SampleCfg) == SampleCfg.seed.offset + 8 + 16
    assert SampleCfg.forced_mode.offset == SampleCfg.seed.offset + 16
    from voicecraft_amd._lib import DebugAttnArgs
    # ten pointers, nine int32, tail padding to the pointers' alignment
    assert DebugAttnArgs.dtype.offset == 80 and DebugAttnArgs.part16.offset == 112 and C.sizeof(DebugAttnArgs) == 120
    from voicecraft_amd._lib import DebugTileAttnArgs
    # seven pointers, six int32
    assert DebugTileAttnArgs.x_out.offset == 48 and DebugTileAttnArgs.dtype.offset == 56 and DebugTileAttnArgs.form.offset == 76
    assert C.sizeof(DebugTileAttnArgs) == 80


def test_debug_attn_refuses_what_no_decode_pass_issues(lib):
    """vc_debug_attn checks its arguments before it touches the device: the refusals need no GPU (the pointers are never read)."""
    from voicecraft_amd._lib import DebugAttnArgs

    def args(**kw):
        base = dict(q=16, kcache=32, vcache=48, row_seq=4, row_pos=8, n_active=12, share_len=20, att_o=64, att_ml=80, x_out=None,
                    dtype=1, H=2, hd=64, S_max=128, rows=3, nsplit=4, nt=0, fast=1, part16=0)
        base.update(kw)
        return DebugAttnArgs(**base)

    bad = [dict(hd=48), dict(hd=256), dict(hd=0), dict(nsplit=0), dict(nsplit=9), dict(x_out=96), dict(x_out=96, nsplit=2),
           dict(part16=1, dtype=0), dict(part16=1, x_out=96, nsplit=1), dict(dtype=2), dict(rows=0), dict(H=0), dict(S_max=0),
           dict(q=None), dict(kcache=None), dict(vcache=None), dict(row_seq=None), dict(row_pos=None), dict(n_active=None),
           dict(share_len=None), dict(att_o=None), dict(att_ml=None), dict(q=20), dict(kcache=40)]
    for kw in bad:
        assert lib.vc_debug_attn(C.byref(args(**kw)), None) == -1, kw
    assert lib.vc_debug_attn(None, None) == -1


def test_debug_tile_attn_refuses_what_no_prefill_pass_issues(lib):
    """vc_debug_tile_attn checks its arguments before it touches the device: the refusals need no GPU (the pointers are never read)."""
    from voicecraft_amd._lib import DebugTileAttnArgs

    def args(**kw):
        base = dict(q=16, kcache=32, vcache=48, row_seq=4, row_pos=8, share_len=20, x_out=64, dtype=1, H=2, hd=128, S_max=128, rows=64, form=1)
        base.update(kw)
        return DebugTileAttnArgs(**base)

    bad = [dict(hd=48), dict(hd=256), dict(hd=0), dict(form=0), dict(form=3), dict(form=2, dtype=0), dict(form=2, hd=64), dict(form=2, hd=32),
           dict(rows=0), dict(rows=-16), dict(rows=8), dict(rows=24), dict(form=2, rows=16), dict(form=2, rows=96), dict(dtype=2), dict(dtype=-1),
           dict(H=0), dict(S_max=0), dict(q=None), dict(kcache=None), dict(vcache=None), dict(row_seq=None), dict(row_pos=None),
           dict(share_len=None), dict(x_out=None), dict(q=20), dict(kcache=40), dict(vcache=56), dict(x_out=72)]
    for kw in bad:
        assert lib.vc_debug_tile_attn(C.byref(args(**kw)), None) == -1, kw
    assert lib.vc_debug_tile_attn(None, None) == -1


def test_no_device_fails_loudly(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from voicecraft_amd import synth
    from voicecraft_amd._lib import ModelCfg
    a = synth.make_args("tiny")
    cfg = ModelCfg(d_model=a.d_model, nhead=a.nhead, num_layers=a.num_decoder_layers, n_codebooks=4,
                   audio_vocab_size=2048, n_special=4, text_rows=101, head_hidden=1024, empty_token=2048, eog=2049,
                   audio_pad_token=2050, eos=2051, reduced_eog=1, encodec_sr=50, max_n_spans=3, max_seqs=2, max_positions=256)
    h = C.c_void_p()
    rc = lib.vc_create(C.byref(cfg), 0, C.byref(h))
    assert rc == -3 and not h.value                      # VC_EHIP, no engine
    assert b"hipSetDevice" in lib.vc_last_error(None)
    from voicecraft_amd.engine import VoiceCraftEngine
    with pytest.raises(RuntimeError):
        VoiceCraftEngine(a, {}, device="cpu")


def test_bad_config_is_rejected(lib):
    from voicecraft_amd._lib import ModelCfg
    cfg = ModelCfg(d_model=300, nhead=4, num_layers=1, n_codebooks=4, audio_vocab_size=2048, n_special=4, text_rows=101,
                   head_hidden=1024, empty_token=2048, eog=2049, audio_pad_token=2050, eos=2051, reduced_eog=1,
                   encodec_sr=50, max_n_spans=3, max_seqs=1, max_positions=256)
    h = C.c_void_p()
    assert lib.vc_create(C.byref(cfg), 0, C.byref(h)) == -1
    assert b"d_model" in lib.vc_last_error(None)


def _cfg(**kw):
    from voicecraft_amd._lib import ModelCfg
    base = dict(d_model=256, nhead=4, num_layers=1, n_codebooks=4, audio_vocab_size=2048, n_special=4, text_rows=101,
                head_hidden=1024, empty_token=2048, eog=2049, audio_pad_token=2050, eos=2051, reduced_eog=1,
                encodec_sr=50, max_n_spans=3, max_seqs=1, max_positions=256)
    base.update(kw)
    return ModelCfg(**base)


def test_one_codebook_is_refused_with_the_reason(lib):
    """K = 1: the reference's TTS cuts the shifted prompt with [:, :-(n_codebooks-1)] = [:, :-0] and so drops the whole audio
    prompt (models/voicecraft.py:967, :1217); the engine keeps it, so there is no parity to offer.  vc_create and the Python
    mirror refuse; the engine-less pattern entry points keep K = 1 (their argument checks still pass for it)."""
    h = C.c_void_p()
    assert lib.vc_create(C.byref(_cfg(n_codebooks=1)), 0, C.byref(h)) == -1 and not h.value
    msg = lib.vc_last_error(None)
    assert b"n_codebooks 1" in msg and b"prompt" in msg, msg
    assert lib.vc_create(C.byref(_cfg(n_codebooks=0)), 0, C.byref(h)) == -1 and not h.value
    assert lib.vc_create(C.byref(_cfg(n_codebooks=9)), 0, C.byref(h)) == -1 and not h.value
    assert b"n_codebooks 9" in lib.vc_last_error(None)
    from voicecraft_amd import synth
    from voicecraft_amd.engine import VoiceCraftEngine
    with pytest.raises(AssertionError, match="n_codebooks 1 unsupported.*prompt"):
        VoiceCraftEngine(synth.make_args("tiny", n_codebooks=1), {}, device="cuda:0")
    assert lib.vc_pattern_unshift(None, 1, 1, None, None) == 0       # N == K == 1: accepted, nothing to write
    assert lib.vc_pattern_shift(None, 1, 1, 3, 0, None, None) == -1  # (null pointers are what is refused here, not K = 1)


def test_vocabulary_and_head_width_limits(lib):
    """V = audio_vocab_size + n_special may be at most 2176 (64 lanes x 34 logits in the sampler); head_hidden a multiple of 256."""
    h = C.c_void_p()
    assert lib.vc_create(C.byref(_cfg(n_special=129)), 0, C.byref(h)) == -1 and not h.value            # V = 2177
    assert b"2177" in lib.vc_last_error(None) and b"2176" in lib.vc_last_error(None)
    assert lib.vc_create(C.byref(_cfg(head_hidden=384)), 0, C.byref(h)) == -1 and not h.value
    assert b"head_hidden 384" in lib.vc_last_error(None)
    # the limits themselves pass the argument checks: what is left to fail without a GPU is the device, with a GPU nothing
    for ok in (_cfg(n_special=128), _cfg(head_hidden=768, audio_vocab_size=1536, empty_token=1536, eog=1537, audio_pad_token=1538, eos=1539),
               _cfg(n_codebooks=2), _cfg(n_codebooks=8)):
        rc = lib.vc_create(C.byref(ok), 0, C.byref(h))
        assert rc in (0, -3), (rc, lib.vc_last_error(None))
        if rc == 0:
            lib.vc_destroy(h)
            h = C.c_void_p()


def test_pattern_entry_points_validate_arguments(lib):
    assert lib.vc_pattern_shift(None, 1, 4, 3, 0, None, None) == -1
    assert lib.vc_pattern_unshift(None, 2, 4, None, None) == -1      # N < K
    assert lib.vc_pattern_unshift(None, 4, 4, None, None) == 0       # N == K: nothing to write
