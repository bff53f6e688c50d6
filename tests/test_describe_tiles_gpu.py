"""k_describe's tiling: a workgroup takes 64 consecutive keypoint slots of one image, eight at
a time, with the per-keypoint angle / sincos / output position done one slot per lane between
the moments and the descriptors.  Every case runs the public extractor and a batch plan and
compares keypoints (every field, the angle by its bits) and descriptors with the CPU oracle.

The inputs are 221 x 221, the smallest square for which level 7 (62 x 62) still has a FAST
cell.  Each case asserts, from the oracle, that its input has the property it is there for.
A level's slots are [kp_off, kp_off + cap) with cap = max(features_per_level + 3, 4 nIni + 4)
(nIni = 1 for a square frame); the retained keypoints fill the first slots of each range.
"""
import ctypes as C

import numpy as np
import pytest

from ar_orbslam2_amd import ORBextractor, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

S = 221
TILE = 64


def _dots(n):
    """n isolated dots 26 above a gentle ramp: with iniThFAST = minThFAST = 20 each is one
    level-0 keypoint and nothing else is (the oracle's count is asserted by the caller)."""
    yy, xx = np.mgrid[0:S, 0:S]
    img = (60 + (xx + 2 * yy) // 8).astype(np.uint8)
    for i in range(n):
        img[25 + 12 * (i // 14), 25 + 12 * (i % 14)] += 26
    return img


def _level_gap():
    """Dots that fade out by level 3 and broad Gaussian blobs that only become corners from
    level 5 on: level 4 retains nothing."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    img = np.full((S, S), 60.0)
    for cx, cy in ((70, 70), (150, 80), (80, 150), (150, 150), (111, 111)):
        img += 120 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 230.0)
    for _ in range(60):
        y, x = rng.integers(25, S - 25, 2)
        img[y, x] += 40
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _plan_extract(imgs, nf, ini, mn):
    """The images as one batch through a batch plan; returns the plan's slot count per image
    and (keypoints, descriptors) per image."""
    import torch
    from ar_orbslam2_amd import KEYPOINT_DTYPE
    from ar_orbslam2_amd._ffi import Params, check, lib
    n = len(imgs)
    prm = Params(int(nf), 1.2, 8, int(ini), int(mn))
    plan = C.c_void_p()
    check("orbx_plan_create", lib().orbx_plan_create(C.byref(prm), S, S, n, 0, C.byref(plan)))
    try:
        d = torch.from_numpy(np.ascontiguousarray(np.stack(imgs))).cuda()
        check("orbx_plan_extract", lib().orbx_plan_extract(plan, C.c_void_p(d.data_ptr()), n))
        check("orbx_plan_sync", lib().orbx_plan_sync(plan))
        cap = C.c_int32()
        check("orbx_plan_capacity", lib().orbx_plan_capacity(plan, C.byref(cap)))
        kp, ds, ct = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check("orbx_plan_outputs", lib().orbx_plan_outputs(plan, C.byref(kp), C.byref(ds),
                                                            C.byref(ct)))
        hip = C.CDLL("libamdhip64.so")

        def d2h(ptr, nbytes):
            out = np.zeros(nbytes, np.uint8)
            assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0
            return out
        k = cap.value
        counts = d2h(ct.value, 4 * n).view(np.int32)
        kps = d2h(kp.value, n * k * 28).view(KEYPOINT_DTYPE).reshape(n, k)
        desc = d2h(ds.value, n * k * 32).reshape(n, k, 32)
        return k, [(kps[i, :counts[i]].copy(), desc[i, :counts[i]].copy()) for i in range(n)]
    finally:
        lib().orbx_plan_destroy(plan)


def _same(got, ref, what):
    (kps, desc), (okps, odesc) = got, ref
    assert len(kps) == len(okps), (what, len(kps), len(okps))
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        bad = np.nonzero(kps[f] != okps[f])[0]
        assert bad.size == 0, f"{what}: field {f}: {bad.size} differ, first idx {bad[:5]}"
    bad = np.nonzero(kps["angle"].view(np.uint32) != okps["angle"].view(np.uint32))[0]
    assert bad.size == 0, f"{what}: angle: {bad.size} differ, first idx {bad[:5]}"
    if len(okps) == 0:  # the extractor returns no descriptor array for an empty frame
        assert desc is None or len(desc) == 0, what
        return
    assert desc.shape == odesc.shape, what
    bad = np.nonzero((desc != odesc).any(1))[0]
    assert bad.size == 0, f"{what}: descriptors: {bad.size} rows differ, first idx {bad[:5]}"


def _check(imgs, nf, ini, mn):
    """Batch plan (all images at once) and the drop-in extractor (one by one) against the
    oracle; returns the oracle's keypoints per image and the level slot offsets."""
    p = O.params(nf, 1.2, 8, ini, mn)
    refs = [O.extract(img, p) for img in imgs]
    total, got = _plan_extract(imgs, nf, ini, mn)
    fpl = O.tables(p, S, S)["features_per_level"]
    caps = np.maximum(fpl + 3, 8)
    assert caps.sum() == total, "the slot layout this file's tile reasoning assumes"
    for i, (g, r) in enumerate(zip(got, refs)):
        _same(g, r, f"plan image {i}")
    ex = ORBextractor(nf, 1.2, 8, ini, mn)
    for i, (img, r) in enumerate(zip(imgs, refs)):
        _same(ex(img), r, f"extractor image {i}")
    return [r[0] for r in refs], np.concatenate([[0], np.cumsum(caps)])


def test_every_level_has_a_fast_cell_and_no_smaller_square_does():
    assert O.tables(O.params(1000), S, S)["level_w"][7] == 62  # 62 - 2 * 16 = 30: one cell
    assert O.tables(O.params(1000), S - 1, S - 1)["level_w"][7] < 62


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 129])
def test_keypoint_counts_around_a_tile(n):
    """0, one active slot, one short of a tile, a full tile, one into the second tile, one
    into the third: all on level 0, whose slots start at 0."""
    (kps,), off = _check([_dots(n)], 1000, 20, 20)
    assert len(kps) == n and (kps["octave"] == 0).all()
    assert off[1] > 129  # the level's slot range holds them all


def test_tile_spans_level_boundaries():
    """129 keypoints over all eight levels with about 30 slots per level: every tile holds
    active slots of several levels and the inactive tail of each level's range between them."""
    (kps,), off = _check([synth.frame(S, S, 0, 4)], 121, 20, 7)
    per = np.bincount(kps["octave"], minlength=8)
    assert len(kps) == 129 and (per > 0).all()
    spans = 0
    for l in range(1, 8):
        t0 = off[l] - off[l] % TILE  # first slot of the tile that level l starts in
        spans += off[l] % TILE != 0 and off[l - 1] + per[l - 1] > t0
    assert spans >= 4
    assert (per < np.diff(off)).any()  # inactive slots inside tiles


def test_middle_level_without_keypoints():
    (kps,), _ = _check([_level_gap()], 200, 20, 20)
    per = np.bincount(kps["octave"], minlength=8)
    assert per[4] == 0 and per[:4].all() and per[5:].all(), per


def test_batch_of_three_with_different_counts():
    """Cross-image tile indexing and the per-image count: a textured frame, a flat one (no
    keypoints, between the two others) and the level-gap image in one batch."""
    imgs = [synth.frame(S, S, 0, 4), np.full((S, S), 128, np.uint8), _level_gap()]
    kps, _ = _check(imgs, 121, 20, 20)
    n = [len(k) for k in kps]
    assert n[1] == 0 and n[0] > TILE and n[2] > 0 and n[0] != n[2], n
