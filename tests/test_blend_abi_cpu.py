"""The compositing entry points of csrc/blend.hip without a GPU: every entry that validates its arguments refuses, on the host and
before any HIP call, one case per SPLAT_CHECK_ARG line that can be reached without a device -- with SPLAT_E_ARG and the same text
after the "<function>: " prefix of splat_last_error() -- and returns SPLAT_OK for an empty backward.  Device pointers are the dummy
address 16 and are never dereferenced; the HOST tables (set_c0 / set_cn / set_bg, the feature sources, the sets' pointer tables)
are real arrays, because the library reads them.  (The six entries of the file that validate nothing -- the size queries and
splat_blend_sets_uses_forward_pack, which answers 0 for a NULL table -- have no case here.)"""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ONE = ctypes.c_void_p(16)          # never dereferenced: every call of these tests ends on the host
E_ARG, OK = -1, 0
NULL_PTR = "null pointer"
DETERMINISTIC = ("the backward needs this library's pair map (goff_incl, slot_sorted, pair_scratch); "
                 "a foreign idx_sorted would take the float-atomic kernel")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "splatter_a_video_amd", "csrc"), "-j8"])
    import splatter_a_video_amd._lib as L
    return L.lib()


def i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def f32(*v):
    return (ctypes.c_float * len(v))(*v)


def i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def ptrs(*v):
    """a host table of device pointers (None = NULL)"""
    return (ctypes.c_void_p * len(v))(*[16 if x else None for x in v])


def call(lib, name, defaults, **override):
    """the entry point `name` with `defaults` (argument name -> value, in the prototype's order) and some arguments replaced"""
    unknown = set(override) - set(defaults)
    assert not unknown, unknown
    return getattr(lib, name)(*dict(defaults, **override).values())


def refused(lib, name, defaults, text, **override):
    rc = call(lib, name, defaults, **override)
    err = lib.splat_last_error().decode()
    assert rc == E_ARG, (name, override, rc, err)
    assert ": " in err and err.split(": ", 1)[1] == text, (name, override, err)


def each_null(lib, name, defaults, keys, text=NULL_PTR):
    for k in keys:
        refused(lib, name, defaults, text, **{k: None})


TOO_MANY = dict(F=1 << 10, W=1 << 16, H=1 << 16)     # 2^10 frames of 2^24 tiles

# ---------------------------------------------------------------- single frame
FWD = dict(P=10, C=3, uv=ONE, conic=ONE, opacity=ONE, feature=ONE, bias=None, idx=ONE, tr=ONE, bg=0.0, bgc=None, W=64, H=48, K=0,
           trunc=0, out=ONE, fT=ONE, nc=ONE, gs_idx=None, pack=ONE, stream=None)
FWD_FLAGS = dict(list(FWD.items())[:-1], cull=ONE, stream=None)
BWD = dict(P=10, C=3, uv=ONE, conic=ONE, opacity=ONE, feature=ONE, bias=None, idx=ONE, tr=ONE, bg=0.0, W=64, H=48, fT=ONE, nc=ONE,
           g=ONE, d_uv=ONE, d_abs_uv=None, d_conic=ONE, d_opacity=ONE, d_feature=ONE, d_bias=None, d_ndc=None, d_abs_ndc=None,
           goff=ONE, slot=ONE, pair=ONE, pack=ONE, pack_valid=0, dbg=None, stream=None)
BWD_FLAGS = dict(list(BWD.items())[:-1], cull=ONE, stream=None)


@pytest.mark.parametrize("name,args", [("splat_alpha_blending_forward", FWD), ("splat_alpha_blending_forward_flags", FWD_FLAGS)])
def test_single_frame_forward(lib, name, args):
    for bad in (dict(P=-1), dict(C=0), dict(W=0), dict(H=-3)):
        refused(lib, name, args, "bad sizes", **bad)
    each_null(lib, name, args, ("tr", "out", "fT", "nc"))
    each_null(lib, name, args, ("uv", "conic", "opacity", "feature", "pack"))
    each_null(lib, name, dict(args, P=0), ("tr", "out", "fT", "nc"))        # (an empty scene still needs its outputs)


@pytest.mark.parametrize("name,args", [("splat_alpha_blending_backward", BWD), ("splat_alpha_blending_backward_flags", BWD_FLAGS)])
def test_single_frame_backward(lib, name, args):
    for bad in (dict(P=-1), dict(C=0), dict(W=0), dict(H=-3)):
        refused(lib, name, args, "bad sizes", **bad)
    assert call(lib, name, args, P=0) == OK
    assert call(lib, name, args, P=0, uv=None, tr=None, d_uv=None, pack=None) == OK      # nothing else is looked at
    each_null(lib, name, args, ("uv", "conic", "opacity", "feature", "tr", "fT", "nc", "g", "pack"))
    each_null(lib, name, args, ("d_uv", "d_conic", "d_opacity", "d_feature"), "null gradient pointer")
    refused(lib, name, args, "bias given without dL_dopacity_bias", bias=ONE)
    for two in (dict(goff=None), dict(slot=None), dict(pair=None), dict(goff=None, slot=None), dict(slot=None, pair=None)):
        refused(lib, name, args, "goff_incl, slot_sorted and pair_scratch go together", **two)
    no_map = dict(goff=None, slot=None, pair=None)
    refused(lib, name, args, "the tap outputs need the pair-mode backward", d_ndc=ONE, **no_map)
    refused(lib, name, args, "the tap outputs need the pair-mode backward", d_abs_ndc=ONE, d_abs_uv=ONE, **no_map)
    refused(lib, name, args, "dL_dabs_ndc needs dL_dabs_uv", d_abs_ndc=ONE)
    assert not lib.splat_get_deterministic()
    lib.splat_set_deterministic(1)
    try:
        refused(lib, name, args, DETERMINISTIC, **no_map)
        refused(lib, name, args, DETERMINISTIC, bias=ONE, d_bias=ONE, C=40, **no_map)
        refused(lib, name, args, "goff_incl, slot_sorted and pair_scratch go together", goff=None)   # (the earlier line still wins)
    finally:
        lib.splat_set_deterministic(0)
    assert not lib.splat_get_deterministic()


# ---------------------------------------------------------------- frame batch: one row
BATCH_SIZES = (dict(F=0), dict(P=0), dict(C=0), dict(W=0), dict(H=-2), dict(cap=0))
FWD_BATCH = dict(F=3, P=10, C=3, uv=ONE, conic=ONE, opacity=ONE, ofs=0, feature=ONE, ffs=0, idx=ONE, tr=ONE, cap=100, bg=0.0, bgc=None,
                 W=64, H=48, K=0, trunc=0, out=ONE, fT=ONE, nc=ONE, gs_idx=None, pack=ONE, cull=None, stream=None)
BWD_BATCH = dict(F=3, P=10, C=3, idx=ONE, tr=ONE, cap=100, bg=0.0, W=64, H=48, fT=ONE, nc=ONE, g=ONE, want_abs=0, slot=ONE, rec=ONE,
                 pack=ONE, cull=ONE, dbg=None, stream=None)
BWD_SET = dict(F=3, P=10, C=23, c0=4, cn=19, uv=ONE, conic=ONE, opacity=ONE, ofs=0, feature=ONE, ffs=0, idx=ONE, tr=ONE, cap=100,
               bg=0.0, W=64, H=48, fT=ONE, nc=ONE, g=ONE, want_abs=0, slot=ONE, rec=ONE, pack=ONE, dbg=None, stream=None)
FWD_SET = dict(F=3, P=10, C=70, c0=32, cn=32, uv=ONE, conic=ONE, opacity=ONE, ofs=0, feature=ONE, ffs=0, idx=ONE, tr=ONE, cap=100,
               bg=0.0, W=64, H=48, out=ONE, fT=ONE, nc=ONE, pack=ONE, cull=None, stream=None)
BWD_SET_PACKED = dict(F=3, P=10, C=70, c0=64, cn=6, idx=ONE, tr=ONE, cap=100, bg=0.0, W=64, H=48, fT=ONE, nc=ONE, g=ONE, slot=ONE,
                      rec=ONE, pack=ONE, cull=ONE, dbg=None, stream=None)


def test_forward_batch(lib):
    name = "splat_alpha_blending_forward_batch"
    for bad in BATCH_SIZES + (dict(C=33),):
        refused(lib, name, FWD_BATCH, "bad sizes (C <= 32)", **bad)
    each_null(lib, name, FWD_BATCH, ("uv", "conic", "opacity", "feature", "idx", "tr", "out", "fT", "nc", "pack"))
    refused(lib, name, FWD_BATCH, "too many tiles", **TOO_MANY)


def test_backward_batch(lib):
    name = "splat_alpha_blending_backward_batch"
    for bad in BATCH_SIZES + (dict(C=33),):
        refused(lib, name, BWD_BATCH, "bad sizes (C <= 32)", **bad)
    each_null(lib, name, BWD_BATCH, ("idx", "tr", "fT", "nc", "g", "slot", "rec", "pack"))


def test_backward_batch_set(lib):
    name = "splat_alpha_blending_backward_batch_set"
    for bad in BATCH_SIZES:
        refused(lib, name, BWD_SET, "bad sizes", **bad)
    for bad in (dict(c0=-1), dict(cn=0), dict(cn=33, c0=0, C=40), dict(c0=5, cn=19)):
        refused(lib, name, BWD_SET, "the set must be 1..32 channels inside the row", **bad)
    each_null(lib, name, BWD_SET, ("uv", "conic", "opacity", "feature", "idx", "tr", "fT", "nc", "g", "slot", "rec", "pack"))


def test_forward_batch_set(lib):
    name = "splat_alpha_blending_forward_batch_set"
    for bad in BATCH_SIZES + (dict(ofs=-1), dict(ffs=-1)):
        refused(lib, name, FWD_SET, "bad sizes", **bad)
    for bad in (dict(c0=-1), dict(cn=0), dict(cn=33), dict(c0=64, cn=7)):
        refused(lib, name, FWD_SET, "the chunk must be 1..32 channels inside the set", **bad)
    each_null(lib, name, FWD_SET, ("uv", "conic", "opacity", "feature", "idx", "tr", "out", "fT", "nc", "pack"))
    refused(lib, name, FWD_SET, "too many tiles", **TOO_MANY)


def test_backward_batch_set_packed(lib):
    name = "splat_alpha_blending_backward_batch_set_packed"
    for bad in BATCH_SIZES:
        refused(lib, name, BWD_SET_PACKED, "bad sizes", **bad)
    for bad in (dict(c0=-1), dict(cn=0), dict(cn=33, c0=0), dict(c0=64, cn=7)):
        refused(lib, name, BWD_SET_PACKED, "the chunk must be 1..32 channels inside the set", **bad)
    each_null(lib, name, BWD_SET_PACKED, ("idx", "tr", "fT", "nc", "g", "slot", "rec", "pack"))
    refused(lib, name, BWD_SET_PACKED, "too many tiles", **TOO_MANY)


# ---------------------------------------------------------------- frame batch: a row of sources / sets
def sources(L, *rows):
    """(c0, cn, has a feature pointer) per source"""
    tab = (L.FeatureSource * len(rows))()
    for s, (c0, cn, has) in zip(tab, rows):
        s.c0, s.cn, s.feature, s.d_feature, s.frame_stride = c0, cn, 16 if has else None, None, 0
    return tab


FWD_SOURCES = dict(F=3, P=10, C=23, nsrc=3, src=None, uv=ONE, conic=ONE, opacity=ONE, ofs=0, idx=ONE, tr=ONE, cap=100, bgc=ONE,
                   W=64, H=48, K=0, trunc=0, out=ONE, fT=ONE, nc=ONE, gs_idx=None, pack=ONE, cull=None, stream=None)
FWD_SETS = dict(F=3, P=10, C=23, set_c0=None, set_cn=None, set_feature=None, set_ffs=None, uv=ONE, conic=ONE, opacity=ONE, ofs=0,
                idx=ONE, tr=ONE, cap=100, bgc=ONE, W=64, H=48, K=0, trunc=0, out=ONE, fT=ONE, nc=ONE, gs_idx=None, pack=ONE, cull=None,
                stream=None)
# (c0, cn, pointer) rows: what is wrong with them, in the words of the sources entry
BAD_ROWS = [([(0, 3, 1), (3, 1, 1), (4, 20, 1)], "source outside the row / null source pointer"),
            ([(0, 3, 1), (-1, 1, 1), (4, 19, 1)], "source outside the row / null source pointer"),
            ([(0, 3, 1), (3, -1, 1), (4, 19, 1)], "source outside the row / null source pointer"),
            ([(0, 3, 1), (3, 1, 0), (4, 19, 1)], "source outside the row / null source pointer"),
            ([(0, 3, 1), (2, 2, 1), (4, 19, 1)], "the sources overlap"),
            ([(0, 3, 1), (0, 3, 1), (4, 19, 1)], "the sources overlap"),
            ([(0, 3, 1), (2, 2, 1), (4, 19, 0)], "the sources overlap"),              # (a source is checked, then its overlap)
            ([(0, 3, 1), (3, 1, 1), (5, 18, 1)], "the sources do not cover the row's channels"),
            ([(0, 3, 1), (3, 0, 0), (4, 19, 1)], "the sources do not cover the row's channels"),
            ([(1, 3, 1), (4, 1, 1), (5, 18, 1)], "the sources do not cover the row's channels")]


def test_forward_batch_sources(lib):
    import splatter_a_video_amd._lib as L
    name = "splat_alpha_blending_forward_batch_sources"
    args = dict(FWD_SOURCES, src=sources(L, (0, 3, 1), (3, 1, 1), (4, 19, 1)))
    for bad in BATCH_SIZES + (dict(C=33),):
        refused(lib, name, args, "bad sizes (C <= 32)", **bad)
    for bad in (dict(src=None), dict(nsrc=0), dict(nsrc=L.MAX_SOURCES + 1), dict(bgc=None)):
        refused(lib, name, args, "null / oversized source table", **bad)
    each_null(lib, name, args, ("uv", "conic", "opacity", "idx", "tr", "out", "fT", "nc", "pack"))
    for rows, text in BAD_ROWS:
        refused(lib, name, args, text, src=sources(L, *rows))
    full = sources(L, (0, 16, 1), (16, 16, 1))                                          # a row of 32 channels fills the mask
    refused(lib, name, dict(args, C=32, nsrc=2), "the sources overlap", src=sources(L, (0, 16, 1), (15, 17, 1)))
    refused(lib, name, dict(args, C=32, nsrc=2), "the sources do not cover the row's channels", src=sources(L, (0, 16, 1), (17, 15, 1)))
    refused(lib, name, dict(args, C=32, nsrc=2, src=full), "too many tiles", **TOO_MANY)
    refused(lib, name, args, "too many tiles", **TOO_MANY)


def test_forward_batch_sets(lib):
    name, via = "splat_alpha_blending_forward_batch_sets", "splat_alpha_blending_forward_batch_sources"
    args = dict(FWD_SETS, set_c0=i32(0, 3, 4), set_cn=i32(3, 1, 19), set_feature=ptrs(1, 1, 1), set_ffs=i64(0, 0, 0))
    each_null(lib, name, args, ("set_c0", "set_cn", "set_feature", "set_ffs"), "null set table")
    # everything else is the sources entry's refusal, under its name
    refused(lib, name, args, "bad sizes (C <= 32)", C=33)
    assert lib.splat_last_error().decode().startswith(via + ": ")
    refused(lib, name, args, "null / oversized source table", bgc=None)
    each_null(lib, name, args, ("uv", "conic", "opacity", "idx", "tr", "out", "fT", "nc", "pack"))
    for rows, text in BAD_ROWS:
        c0, cn, has = zip(*rows)
        refused(lib, name, args, text, set_c0=i32(*c0), set_cn=i32(*cn), set_feature=ptrs(*has))
    refused(lib, name, args, "too many tiles", **TOO_MANY)


SETS = dict(F=3, P=10, C=23, set_c0=None, set_cn=None, set_bg=None, uv=ONE, conic=ONE, opacity=ONE, ofs=0, feature=ONE, ffs=0,
            set_feature=None, set_ffs=None, idx=ONE, tr=ONE, cap=100, W=64, H=48, fT=ONE, nc=ONE, g=ONE, set_dL=None, want_abs=0,
            slot=ONE, rec=ONE, pack=ONE, cull=ONE, dbg=None, stream=None)
SETS_PACKED = dict(list(SETS.items())[:-1], forward_pack=None, stream=None)
SETS_L1 = dict(F=3, P=10, C=23, set_c0=None, set_cn=None, set_bg=None, uv=ONE, conic=ONE, opacity=ONE, ofs=0, set_feature=None,
               set_ffs=None, idx=ONE, tr=ONE, cap=100, W=64, H=48, fT=ONE, nc=ONE, pred=ONE, set_target=None, l1_scale=None, l1_sum=None,
               want_abs=0, slot=ONE, rec=ONE, pack=ONE, cull=ONE, dbg=None, forward_pack=None, stream=None)


def set_tables(c0=(0, 3, 4), cn=(3, 1, 19)):
    return dict(set_c0=i32(*c0), set_cn=i32(*cn), set_bg=f32(0.2, 1.0, 0.0))


def common_sets_refusals(lib, name, args, own_tensors):
    """the lines of the three-set backward that all three entries reach (own_tensors: the entry has no `feature` / `dL_dout` row)"""
    for bad in BATCH_SIZES + (dict(C=29),):
        refused(lib, name, args, "bad sizes (C <= 28)", **bad)
    each_null(lib, name, args, ("set_c0", "set_cn", "set_bg"), "null set table")
    each_null(lib, name, args, ("uv", "conic", "opacity", "idx", "tr", "fT", "nc", "slot", "rec"))
    for cn in ((5, 1, 17), (-1, 1, 19), (3, 5, 15), (3, -2, 19), (2, 0, 21), (3, 1, -1)):
        refused(lib, name, args, "set widths: tap set <= 4, second set <= 4, detached set <= 20 channels", **set_tables(cn=cn))
    for c0, cn in (((0, 3, 5), (3, 1, 19)), ((-1, 3, 4), (3, 1, 19)), ((0, 20, 4), (3, 4, 19))):
        refused(lib, name, args, "set outside the row", **set_tables(c0, cn))
    for c0, cn in (((0, 2, 4), (3, 2, 19)), ((0, 3, 3), (3, 1, 20)), ((0, 0, 4), (3, 3, 19))):
        refused(lib, name, args, "the sets overlap", **set_tables(c0, cn))
    refused(lib, name, args, "the sets overlap", **set_tables((0, 2, 9), (3, 2, 19)))           # (set 1 overlaps before set 2 is looked at)
    for c0, cn in (((0, 3, 5), (3, 1, 18)), ((0, 3, 4), (3, 0, 19)), ((1, 4, 5), (3, 1, 18)), ((0, 0, 0), (0, 0, 0))):
        refused(lib, name, args, "the sets do not cover the row's channels", **set_tables(c0, cn))
    if own_tensors:
        for k in (0, 1, 2):
            has = [1, 1, 1]
            has[k] = 0
            refused(lib, name, args, "null set feature pointer", set_feature=ptrs(*has))
            refused(lib, name, args, "null set gradient pointer", **{"set_target" if "set_target" in args else "set_dL": ptrs(*has)})


@pytest.mark.parametrize("name,base", [("splat_alpha_blending_backward_batch_sets", SETS),
                                       ("splat_alpha_blending_backward_batch_sets_packed", SETS_PACKED)])
def test_backward_batch_sets(lib, name, base):
    args = dict(base, **set_tables())
    common_sets_refusals(lib, name, args, False)
    refused(lib, name, args, NULL_PTR, pack=None)                                                # (neither scratch nor the forward's records)
    refused(lib, name, args, "features: the row [F,P,C] or the sets' own tensors", feature=None)
    refused(lib, name, args, "features: the row [F,P,C] or the sets' own tensors", feature=None, set_feature=ptrs(1, 1, 1))
    refused(lib, name, args, "features: the row [F,P,C] or the sets' own tensors", feature=None, set_ffs=i64(0, 0, 0))
    refused(lib, name, args, "image gradient: the row [F,C,H,W] or the sets' own tensors", g=None)
    own = dict(args, feature=None, set_feature=ptrs(1, 1, 1), set_ffs=i64(0, 0, 0), g=None, set_dL=ptrs(1, 1, 1))
    common_sets_refusals(lib, name, own, True)
    refused(lib, name, dict(own, **set_tables((0, 3, 0), (3, 1, 0)), C=4), "null set gradient pointer", set_dL=ptrs(1, 0, 0))
    if "forward_pack" in base:
        # the forward's records stand in for the sets' tensors; without the cull words (or under another plan) they do not
        # replace the scratch
        small = dict(args, C=8, **set_tables((0, 3, 4), (3, 1, 4)))
        text = "pack_scratch is needed: the forward's records do not serve this plan / these kernels"
        refused(lib, name, small, text, pack=None, forward_pack=ONE)
        refused(lib, name, args, text, pack=None, forward_pack=ONE, cull=None)
        refused(lib, name, own, text, pack=None, forward_pack=ONE, cull=None, set_feature=ptrs(0, 0, 0))
        refused(lib, name, own, "null set gradient pointer", forward_pack=ONE, set_feature=ptrs(0, 0, 0), set_dL=ptrs(1, 0, 1))


def test_backward_batch_sets_l1(lib):
    name = "splat_alpha_blending_backward_batch_sets_l1"
    args = dict(SETS_L1, **set_tables(), set_feature=ptrs(1, 1, 1), set_ffs=i64(0, 0, 0), set_target=ptrs(1, 1, 1),
                l1_scale=f32(0.8, 0.3, 0.5))
    each_null(lib, name, args, ("pred", "set_target", "l1_scale"))
    assert lib.splat_last_error().decode().startswith(name + ": ")
    fused = ("loss-fused backward: needs the sets' target images, the scales, the forward's cull words and the quarter-list kernels")
    refused(lib, name, args, fused, cull=None)
    import splatter_a_video_amd._lib as L
    with L.option("bwd_quarters", 0):
        refused(lib, name, args, fused)
    assert L.get_option("bwd_quarters") == 1
    common_sets_refusals(lib, name, args, True)
    refused(lib, name, args, NULL_PTR, pack=None)
    refused(lib, name, args, "features: the row [F,P,C] or the sets' own tensors", set_feature=None)
    refused(lib, name, args, "features: the row [F,P,C] or the sets' own tensors", set_ffs=None)
    small = dict(args, C=8, **set_tables((0, 3, 4), (3, 1, 4)))
    refused(lib, name, small, "pack_scratch is needed: the forward's records do not serve this plan / these kernels", pack=None,
            forward_pack=ONE)


# ---------------------------------------------------------------- the records' segment sum
def test_pair_records_segment_sum(lib):
    name = "splat_pair_records_segment_sum"
    args = dict(P=10, ncp=12, rec=ONE, goff=ONE, out=ONE, stream=None)
    for bad in (dict(P=-1), dict(ncp=0), dict(ncp=3), dict(ncp=14), dict(ncp=-4)):
        refused(lib, name, args, "bad sizes (the record stride is a multiple of 4 floats)", **bad)
    assert call(lib, name, args, P=0) == OK
    assert call(lib, name, args, P=0, rec=None, goff=None, out=None) == OK
    each_null(lib, name, args, ("rec", "goff", "out"))
    refused(lib, name, args, "records and out must be 16-byte aligned", rec=ctypes.c_void_p(20))
    refused(lib, name, args, "records and out must be 16-byte aligned", out=ctypes.c_void_p(24))
