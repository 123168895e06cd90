"""The seven w8 requests side by side on bare handles (vc_create needs a device; no GEMM is launched): from every prior state - no
vc_request_w8, or vc_request_w8 of 1, 4 or 5 - every mask -1..16, against one statement of the rule per request, which mirrors what
include/vc_engine.h says of each: which masks exist, whether the mask has to be a subset of vc_request_w8's, and which of the two
refusals comes first.  On a finalized engine every request is VC_ESTATE."""
import ctypes as C

import pytest

from test_w8_rows_cpu import cfg

pytestmark = pytest.mark.gpu

OK, EINVAL, ESTATE = 0, -1, -2
MASKS = range(-1, 17)
PRIOR = (None, 1, 4, 5)           # the mask of an earlier vc_request_w8, None = no such call


def bits_1_4(mask):
    return mask >= 0 and not mask & ~5


# request: (the masks that exist, needs vc_request_w8, the mask is a subset of that request's, the mask is judged before the order,
# masks refused at the end)
REQUESTS = {
    "vc_request_w8": (bits_1_4, False, False, True, ()),
    "vc_request_w8_rows": (bits_1_4, True, True, True, ()),
    "vc_request_w8_wide": (bits_1_4, True, True, True, ()),
    "vc_request_w8_mid": (bits_1_4, True, True, True, (4, 5)),      # bit 4 passes the first two checks and has no form
    "vc_request_w8_up": (lambda m: m == 2, True, False, False, ()),
    "vc_request_w8_up_rows": (lambda m: m == 2, True, False, False, ()),
    "vc_request_w8_qkv_rows": (lambda m: m == 4, True, False, False, ()),
}


def want(name, prior, mask):
    exists, needs_w8, subset, mask_first, late = REQUESTS[name]
    if mask_first and not exists(mask):
        return EINVAL
    if needs_w8 and not prior:
        return ESTATE
    if not exists(mask) or (subset and mask & ~prior) or mask in late:
        return EINVAL
    return OK


@pytest.mark.parametrize("name", sorted(REQUESTS))
def test_every_state_every_mask(name):
    from voicecraft_amd import _lib, synth
    lib = _lib.load()
    a = synth.make_args("tiny128", num_decoder_layers=1)
    c_ = cfg(a.d_model, a.nhead)
    fn = getattr(lib, name)
    for mask in MASKS:
        assert fn(None, mask) == EINVAL
    for prior in PRIOR:
        for mask in MASKS:      # a handle per call: a request that succeeds leaves nothing behind for the next mask
            h = C.c_void_p()
            assert lib.vc_create(C.byref(c_), 0, C.byref(h)) == 0
            try:
                if prior is not None:
                    assert lib.vc_request_w8(h, prior) == OK
                assert fn(h, mask) == want(name, prior, mask), (name, prior, mask)
            finally:
                lib.vc_destroy(h)


def test_finalized_engine_refuses_every_request():
    from voicecraft_amd import synth
    from voicecraft_amd.engine import VoiceCraftEngine
    a = synth.make_args("tiny128", num_decoder_layers=1)
    eng = VoiceCraftEngine(a, synth.make_state_dict(a, seed=0, fast=True), device="cuda:0", dtype="bf16", max_seqs=2, max_positions=64)
    opts = eng.options()
    for name in REQUESTS:
        for mask in MASKS:
            assert getattr(eng.lib, name)(eng._h, mask) == ESTATE, (name, mask)
    assert eng.options() == opts
