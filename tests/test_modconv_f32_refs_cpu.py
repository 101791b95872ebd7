"""CPU check of tests/modconv_f32_refs.py, the tables behind tests/test_hip_modconv_f32_f64.py (the fp32 MFMA conv kernels of
csrc/nb_modconv.hip against float64):
(1) the Python restatement of nb_select_variant names the kernel the library itself names (nb_modconv3x3_variant, host only) over
    the whole case table and a few hundred random shapes;
(2) the table reaches all 11 fp32-output kernels (and with every up = 2 case the five H2OUT twins), each with a ragged last
    slice, several slices and tiles both ways, c_in off the chunk grid with and without a second input, more chunks than ring
    stages and a single chunk, narrow and clipped tiles, all three noise modes and the identity epilogue -- "where the selector
    allows it" is decided by enumerating the selector over a grid of shapes, not by hand;
(3) per case, from the float64 reference alone: every workgroup's block of outputs lies on both sides of kink and clamp, every
    mutation of conv_form_refs.mutations moves the reference by >= CATCH bounds, and a plain fp32 evaluation of the layer on the
    CPU stays within a quarter of the bound the GPU test asserts (2e-6 of max|lin| x gain).
These are conditions on the table and its seeded inputs, not measurements of a kernel."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import conv_form_refs as cf
import modconv_f32_refs as mr


@pytest.fixture(scope="module")
def library():
    from brushstroke_engine_amd import _lib, build
    build.build()
    return _lib.lib()


def _library_name(lib, n, h, w, co, up):
    buf = ctypes.create_string_buffer(128)
    assert lib.nb_modconv3x3_variant(n, h, w, co, up, buf, len(buf)) == 0, lib.nb_last_error()
    return buf.value.decode()


def test_selector_restatement_equals_the_library(library):
    shapes = [(c.n, c.h, c.w, c.co, c.up) for c in mr.CASES]
    rs = np.random.RandomState(384)
    for _ in range(600):
        # batches, channels and image sizes on both sides of every threshold of the selector (the target of 384 workgroups)
        shapes.append((int(rs.choice([1, 2, 3, 5, 8, 12, 24, 47, 96, 192, 383, 384, 768, 4000])), 4 << int(rs.randint(0, 7)), 4 << int(rs.randint(0, 7)),
                       int(rs.choice([1, 8, 16, 17, 32, 33, 40, 64, 65, 72, 128, 129, 136, 200, 512])), int(rs.randint(1, 3))))
    seen = set()
    for n, h, w, co, up in shapes:
        v, tq = mr.select_variant(n, h, w, co, up)
        assert _library_name(library, n, h, w, co, up) == mr.kernel_name(v), (n, h, w, co, up)
        assert (tq is None) == (up == 1) and (up == 1 or mr.UP2_KERNELS[v][0] == _nbp_of(tq))
        seen.add(v)
    assert seen == set(mr.UP1_KERNELS) | set(mr.UP2_KERNELS)


def _nbp_of(tq):
    """The instantiation (NBP) the selector's thresholds give a quad tile."""
    nbp = mr.up2_blocks(*tq)
    return 10 if nbp > 6 else 6 if nbp > 3 else 3 if nbp > 2 else 2 if nbp > 1 else 1


def test_table_names_the_kernel_each_case_reaches():
    for c in mr.CASES:
        assert mr.select_variant(c.n, c.h, c.w, c.co, c.up) == (c.variant, c.tq), mr.case_id(c)
        assert c.c1 > 0 and c.c2 >= 0 and c.c1 + c.c2 <= mr.STY_MAX
        if c.up == 1:
            assert mr.up1_geometry(c.variant, c.h, c.w)[4], f"{mr.case_id(c)}: the launcher refuses this tile"
        else:
            assert c.h % c.tq[0] == 0 and c.w % c.tq[1] == 0 and mr.up2_blocks(*c.tq) <= mr.UP2_KERNELS[c.variant][0]
    assert len(set(mr.CASES)) == len(mr.CASES)


def _features(up, v, tq, n, co, h, w):
    """What a launch's geometry offers: the flags the table must show per kernel."""
    if up == 1:
        tw, th, cs, pix, fits = mr.up1_geometry(v, h, w)
        if not fits:
            return None
        ty, tx, clipped, narrow = -(-h // th), w // tw, th < pix // tw, w < 32
    else:
        cs, ty, tx, clipped, narrow = 16, h // tq[0], w // tq[1], tq not in mr.UP2_TILES, False
    sl = -(-co // cs)
    return dict(rows=ty >= 2, cols=tx >= 2, slices=sl >= 2, all3=ty >= 2 and tx >= 2 and sl >= 2, clipped=clipped, narrow=narrow,
                tq=tq)


@functools.lru_cache(maxsize=None)
def _selector_allows():
    """kernel -> the set of (feature, value) some shape of a wide grid reaches it with."""
    out = {}
    for up in (1, 2):
        for n in (1, 2, 3, 5, 6, 12, 16, 24, 48, 96, 192, 384, 768, 3000):
            for co in (8, 20, 24, 36, 40, 72, 136, 200, 520):
                for h in (4, 8, 16, 32, 64, 128, 256):
                    for w in (4, 8, 16, 32, 64, 128, 256):
                        v, tq = mr.select_variant(n, h, w, co, up)
                        f = _features(up, v, tq, n, co, h, w)
                        if f:
                            out.setdefault(v, set()).update((k, x) for k, x in f.items() if x)
    return out


@pytest.mark.parametrize("v", sorted(set(mr.UP1_KERNELS) | set(mr.UP2_KERNELS)))
def test_table_meets_every_condition_per_kernel(v):
    cases = [c for c in mr.CASES if c.variant == v]
    assert cases, "kernel not reached"
    up = cases[0].up
    kc, nst = mr.kc_nst(v)
    ci = lambda c: c.c1 + c.c2
    if up == 1:
        assert any(c.co % 32 for c in cases)
    else:
        assert any(c.co % 16 and c.co % 8 for c in cases)                           # (a last slice that ends inside an H2 group of 8)
    got = set()
    for c in cases:
        got.update((k, x) for k, x in _features(c.up, c.variant, c.tq, c.n, c.co, c.h, c.w).items() if x)
    missing = _selector_allows()[v] - got
    assert not missing, f"the selector allows {sorted(missing, key=str)} on this kernel and the table has no such case"
    assert any(ci(c) % kc and c.c2 > 0 and c.c1 % 4 for c in cases) and any(ci(c) % kc and c.c2 == 0 for c in cases)
    assert any(c.c2 > 0 and c.c1 % 4 == 0 for c in cases)
    assert any(ci(c) > kc * nst and ci(c) % kc for c in cases) and any(ci(c) <= kc for c in cases)
    assert {c.noise for c in cases if c.epi == "live"} == {"per", "shared", "null"}
    assert any(c.epi == "identity" and c.noise == "null" for c in cases)
    if up == 2:
        assert all(mr.h2_allowed(c) for c in cases)


def test_what_the_selector_allows():
    """The enumeration itself, written out: <8,2,2,4,3> never has a second slice (33 .. 64 channels in workgroups of 64), no clipped
    tile reaches <4,1,1,8,4> or <10,4>, and the clipped quad tiles are exactly these."""
    a = _selector_allows()
    assert ("slices", True) not in a[1] and ("clipped", True) not in a[4] and ("clipped", True) not in a[5]
    tiles = {v: {x for k, x in a[v] if k == "tq"} for v in mr.UP2_KERNELS}
    assert tiles == {5: {(16, 32)}, 6: {(16, 16), (8, 32), (4, 32)}, 7: {(8, 16), (16, 8)}, 8: {(8, 8), (4, 16), (16, 4)},
                     9: {(4, 4), (4, 8), (8, 4)}}
    for v in (0, 1, 2, 3, 10):
        assert {("narrow", True), ("clipped", True)} <= a[v]


@pytest.mark.parametrize("c", mr.CASES, ids=mr.case_id)
def test_case_meets_kink_and_clamp_catches_mutations_and_fp32_has_room(c):
    up, n, ci, co, h, w = mr.shape_of(c)
    d, r = cf.inputs(up, n, ci, co, h, w), mr.reference(c)
    th, tw, cs = mr.block_of(c)
    bound = mr.B * r["scale"]
    # the plain fp32 evaluation: the bound has room for another summation order
    err = float((mr.evaluate_f32(c).double() - r["ref"]).abs().max())
    print(f"[modconv-f32] {mr.case_id(c)}: plain fp32 on the CPU {err:.3e} = {err / r['scale']:.3e} of max|lin| x gain, {err / bound:.3f} of the bound")
    assert err <= mr.QUARTER * bound, f"plain fp32 evaluation at {err / bound:.3f} of the bound: change the case"
    loosest = bound
    if mr.h2_allowed(c):
        want = cf.handoff_want(d, r["ref"], co)
        loosest = max(loosest, cf.tol_handoff(0, r["scale"], d, want, co))
    if c.epi == "live":
        bad = cf.blocks_meet_kink_and_clamp(r["pre"], r["act"], th, tw, cs)
        assert not bad, f"blocks (sample, channel, row, column) that miss the kink or the clamp: {bad[:8]} ({len(bad)})"
        muts = cf.mutations(up, n, ci, co, h, w, c.noise, th)
    else:
        muts = mr.identity_mutations(c)
    for name, m in muts.items():
        moved = float((m - r["ref"]).abs().max())
        assert moved >= cf.CATCH * loosest, f"{name}: moves the reference by {moved:.3e}, bound {loosest:.3e}"
