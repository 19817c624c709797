"""CPU checks of the batch layout generator (tests/layouts.py) over the pinned seeds of tests/test_gpu_layouts.py: planes
never overlap and lie inside their frame, the guard mask and the plane views partition each buffer exactly, and every
layout class the generator promises appears.  If a change to the generator loses coverage, this fails without a GPU."""
import numpy as np
import pytest

from tests import layouts as LY

ALL_SEEDS = sorted(set(LY.SEEDS) | set(LY.PIPE_SEEDS) | set(LY.POSED_SEEDS) | set(LY.FUSED_SEEDS))


@pytest.fixture(scope="module")
def drawn():
    return [LY.draw_layout(s) for s in ALL_SEEDS]


def _rects(L, side):
    out = []
    for p in L.planes:
        if side == "in":
            out.append((p.in_off, p.in_w, p.in_h, p.in_stride))
        else:
            out.append((p.out_off, p.out_w, p.out_h, p.out_stride))
    return out


@pytest.mark.parametrize("side", ["in", "out"])
def test_planes_lie_inside_their_frame_and_never_overlap(side, drawn):
    for L in drawn:
        fb = L.in_frame_bytes if side == "in" else L.out_frame_bytes
        assert fb >= LY.extent(L, side), (L.seed, side)
        frame = np.zeros(fb, np.int32)
        for off, w, h, s in _rects(L, side):
            assert off >= 0 and s >= w > 0 and h > 0
            assert off + (h - 1) * s + w <= fb, (L.seed, side)
            for y in range(h):
                frame[off + y * s:off + y * s + w] += 1
        assert frame.max() == 1, "seed %d: planes of one %s frame overlap" % (L.seed, side)
        assert (fb if L.n_frames > 1 else 0) * (L.n_frames - 1) + LY.extent(L, side) + (L.in_base if side == "in" else L.out_base) \
            < (L.in_bytes if side == "in" else L.out_bytes)


def test_guard_mask_and_plane_views_partition_the_buffers(drawn):
    for L in drawn:
        for side in ("in", "out"):
            nbytes = L.in_bytes if side == "in" else L.out_bytes
            buf = np.arange(nbytes, dtype=np.int64)   # byte i holds i: a view names exactly the bytes it covers
            count = np.zeros(nbytes, np.int32)
            for f in range(L.n_frames):
                for k in range(len(L.planes)):
                    v = L.plane_view(buf, f, k, side)
                    p = L.planes[k]
                    assert v.shape == ((p.in_h, p.in_w) if side == "in" else (p.out_h, p.out_w))
                    np.add.at(count, v.ravel(), 1)
            assert count.max() == 1, "seed %d: two plane views share a byte" % L.seed
            cov = L.covered(side)
            assert np.array_equal(cov, count == 1)
            if side == "out":
                guard = L.guard_mask()
                assert np.array_equal(guard, count == 0) and guard.sum() + cov.sum() == nbytes
                # the bytes before frame 0 and after the last frame are guarded
                assert guard[:L.out_base].all() and guard[-LY.SLACK:].all()


def test_every_layout_class_appears(drawn):
    seen = {k: set() for k in ("in_base", "out_base", "in_stride", "out_stride", "in_width", "out_width", "in_frame",
                               "out_frame", "planes", "frames")}
    out_w_not4 = many_maps = scaled = tiled_in = fast_out = 0
    for L in drawn:
        seen["in_base"].add(L.in_base % 16)
        seen["out_base"].add(L.out_base % 16)
        seen["planes"].add(len(L.planes))
        seen["frames"].add(L.n_frames)
        assert L.in_frame_bytes != L.out_frame_bytes
        if L.n_frames > 1:
            seen["in_frame"].add(LY.frame_class(L.in_frame_bytes, LY.extent(L, "in")))
            seen["out_frame"].add(LY.frame_class(L.out_frame_bytes, LY.extent(L, "out")))
        for p in L.planes:
            seen["in_stride"].add(LY.stride_class(p.in_stride, p.in_w))
            seen["out_stride"].add(LY.stride_class(p.out_stride, p.out_w))
            seen["in_width"].add(LY.width_class(p.in_w))
            seen["out_width"].add(LY.width_class(p.out_w))
            out_w_not4 += p.out_w % 4 != 0
            # each plane has its map's size
            assert L.maps[p.map_idx] == (p.in_w, p.in_h, p.out_w, p.out_h)
            assert p.in_w * p.in_h <= 640 * 320 and p.out_w * p.out_h <= 384 * 256
        many_maps += any(p.map_idx >= 2 for p in L.planes)
        scaled += L.scaled()
        # both sides of the 16-byte source gate and of the dword store gate
        tiled_in += L.in_base % 16 == 0 and all(p.in_stride % 16 == 0 and p.in_w % 16 == 0 and p.in_off % 16 == 0 for p in L.planes) \
            and (L.n_frames == 1 or L.in_frame_bytes % 16 == 0)
        fast_out += L.out_base % 4 == 0 and all(p.out_stride % 4 == 0 and p.out_off % 4 == 0 for p in L.planes) \
            and (L.n_frames == 1 or L.out_frame_bytes % 4 == 0)
    assert seen["in_base"] >= set(LY.BASE_CLASSES) and seen["out_base"] >= set(LY.BASE_CLASSES), seen
    for k in ("in_stride", "out_stride"):
        assert seen[k] >= set(LY.STRIDE_CLASSES), (k, seen[k])
    for k in ("in_width", "out_width"):
        assert seen[k] >= set(LY.WIDTH_CLASSES), (k, seen[k])
    for k in ("in_frame", "out_frame"):
        assert seen[k] >= set(LY.FRAME_CLASSES), (k, seen[k])
    assert seen["planes"] >= set(LY.PLANE_COUNTS), seen["planes"]
    assert seen["frames"] >= set(LY.FRAME_COUNTS), seen["frames"]
    assert out_w_not4 > 0 and many_maps >= 2
    n = len(drawn)
    assert n // 8 <= scaled <= n // 2, "%d of %d layouts have scale factors" % (scaled, n)
    assert n // 8 <= tiled_in < n and n // 8 <= fast_out < n, (tiled_in, fast_out, n)


def test_pinned_seed_lists_have_what_their_tests_need():
    fused = [LY.draw_layout(s) for s in LY.FUSED_SEEDS]
    assert fused and all(L.fusable() for L in fused)
    posed = [LY.draw_layout(s) for s in LY.POSED_SEEDS]
    assert sum(L.posed_eligible() for L in posed) >= len(posed) // 2
    assert any(not L.posed_eligible() for L in posed)
    assert any(L.n_frames > 64 for L in posed) and any(len(L.planes) > 4 for L in posed)
    assert any(p.out_w % 4 for L in posed for p in L.planes)


def test_pinned_layouts_have_maps(drawn, oracle_mod):
    """every map of every pinned layout is one the oracle generates (a refused map would leave a GPU test nothing to
    compare)"""
    for L in drawn:
        o = oracle_mod.Oracle(L.ctx())
        try:
            for idx, d in L.maps.items():
                assert o.generateMapForPlane(*d, idx), (L.seed, idx, d)
        finally:
            o.close()


def test_layouts_are_reproducible():
    for s in (0, 7, 123):
        a, b = LY.draw_layout(s), LY.draw_layout(s)
        assert a == b
