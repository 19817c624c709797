"""Seeded memory layouts for the batch entry points (T360_transformFrames, T360_transformFramesPipelined,
T360_transformFramesPosed).

A T360PlaneDesc batch may place its planes anywhere: any byte offset of the input and output base, any row stride, any
frame stride and any number of planes.  The host code picks kernels and store widths from the alignment of that layout
(the 16-byte DMA source of the tiled gather, the raw plane of the fused low-pass, dword or byte stores, groups of 4
planes per launch, 64-frame posed chunks), so draw_layout(seed) sends a batch through both sides of every such gate:

  base offset mod 16     0, 1, 4, 8 (input and output drawn separately)
  row stride             the width; the width + an odd pad of 1-15; a multiple of 16
  plane width            a multiple of 16; a multiple of 4 but not of 16; odd (input and output widths)
  frame stride           tight (the planes and their gaps, often odd); a multiple of 4 but not of 16; a multiple of 256
  planes                 1, 2, 3, 4, 5, 8; maps 0 and 1, in a few seeds maps 2-7
  frames                 1, 2, 23, 24, 25, 63, 64, 65, 129 (small counts weighted up)

Planes never overlap, and every plane has its map's size.  The contexts come from tests/test_gpu_fuzz.draw (scale factors
in about a quarter of them).  tests/test_layouts_cpu.py checks the generator and its coverage without a GPU;
tests/test_gpu_layouts.py and tests/soak/layout_soak.py run the layouts on the device.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from transform360_amd import _lib
from transform360_amd.abi import (CUBIC, LINEAR, STEREO_FORMAT_MONO, filter_defaults)

SENTINEL = 0x5A
BASE_CLASSES = (0, 1, 4, 8)
STRIDE_CLASSES = ("tight", "odd_pad", "mult16")
WIDTH_CLASSES = ("mult16", "mult4", "odd")
FRAME_CLASSES = ("tight", "mult4", "mult256")
PLANE_COUNTS = (1, 2, 3, 4, 5, 8)
FRAME_COUNTS = (1, 2, 23, 24, 25, 63, 64, 65, 129)
_FRAME_WEIGHTS = np.array([8, 6, 3, 3, 3, 1.5, 1.5, 1.5, 1.0])
_PLANE_WEIGHTS = np.array([2, 2, 4, 2, 2, 1.5])
ORACLE_THREADS = 8  # threads of each oracle handle (the soak runs several processes side by side with fewer)
SLACK = 61  # bytes after the last frame's last plane: guard bytes of the tail

# the pinned seeds of the suite (tests/test_gpu_layouts.py); tests/test_layouts_cpu.py checks their class coverage
SEEDS = list(range(40)) + [97]                 # 97: 129 frames
PIPE_SEEDS = list(range(12))
POSED_SEEDS = list(range(20)) + [25, 97]       # 25: 65 frames of 5 planes
# fusable draws (Layout.fusable): the first 16 below 300, and 552 (8 planes, 16-byte friendly source)
FUSED_SEEDS = [8, 19, 30, 33, 121, 123, 141, 149, 166, 186, 201, 245, 257, 279, 281, 293, 552]


@dataclass
class Plane:
    map_idx: int
    in_w: int
    in_h: int
    out_w: int
    out_h: int
    in_stride: int
    out_stride: int
    in_off: int = 0    # inside the frame
    out_off: int = 0


@dataclass
class Layout:
    seed: int
    ov: dict
    planes: list
    maps: dict               # map index -> (in_w, in_h, out_w, out_h) for generateMapForPlane
    n_frames: int
    in_frame_bytes: int
    out_frame_bytes: int
    in_base: int             # offset of frame 0 from the 256-byte aligned allocation
    out_base: int
    in_bytes: int            # allocation sizes, base offset and tail slack included
    out_bytes: int
    classes: dict = field(default_factory=dict)

    def ctx(self):
        return filter_defaults(**self.ov)

    def descs(self):
        arr = (_lib.T360PlaneDesc * len(self.planes))()
        for k, p in enumerate(self.planes):
            arr[k] = _lib.T360PlaneDesc(in_offset=p.in_off, out_offset=p.out_off, in_stride=p.in_stride,
                                        out_stride=p.out_stride, in_width=p.in_w, in_height=p.in_h,
                                        out_width=p.out_w, out_height=p.out_h, map_index=p.map_idx)
        return arr

    def scaled(self):
        return self.ov.get("width_scale_factor", 1.0) != 1.0 or self.ov.get("height_scale_factor", 1.0) != 1.0

    def posed_eligible(self):
        """T360_transformFramesPosed takes the context: no scale factors, no pose-dependent (adjust_kernel) low-pass"""
        return not self.scaled() and not (self.ov.get("enable_low_pass_filter", 1) and self.ov.get("adjust_kernel", 1))

    def fusable(self):
        """what T360_setFusedLowpass can fuse: a MONO low-pass context, LINEAR or CUBIC, a long batch"""
        ov = self.ov
        return (ov.get("enable_low_pass_filter", 1) == 1 and ov.get("input_stereo_format", STEREO_FORMAT_MONO) == STEREO_FORMAT_MONO
                and ov.get("interpolation_alg", CUBIC) in (LINEAR, CUBIC) and self.n_frames >= 24 and not self.scaled())

    def sample_frames(self):
        """frames 0, 1 and the last, and either side of 24 (the long-batch plan), 64 (a workgroup's frames, the posed
        chunk) and of the halves a launch splits its frames into"""
        n = self.n_frames
        half = (n + 1) // 2
        want = {0, 1, n - 1, 23, 24, 63, 64, half - 1, half}
        return sorted(f for f in want if 0 <= f < n)

    # ---- buffers ----
    def _span(self, side, f, k):
        p = self.planes[k]
        if side == "in":
            return self.in_base + f * self.in_frame_bytes + p.in_off, p.in_w, p.in_h, p.in_stride
        return self.out_base + f * self.out_frame_bytes + p.out_off, p.out_w, p.out_h, p.out_stride

    def plane_view(self, buf, f, k, side="out"):
        """2-D (h, w) view of plane k of frame f inside the whole host buffer `buf` (one element per byte, allocation
        start)"""
        start, w, h, s = self._span(side, f, k)
        assert buf.ndim == 1 and start + (h - 1) * s + w <= buf.size
        b = buf.itemsize
        return np.lib.stride_tricks.as_strided(buf[start:], shape=(h, w), strides=(s * b, b), writeable=False)

    def covered(self, side="out", n_frames=None):
        """boolean mask of the bytes of the buffer that some plane of some frame covers"""
        n = self.n_frames if n_frames is None else n_frames
        m = np.zeros(self.in_bytes if side == "in" else self.out_bytes, bool)
        for f in range(n):
            for k in range(len(self.planes)):
                start, w, h, s = self._span(side, f, k)
                np.lib.stride_tricks.as_strided(m[start:], shape=(h, w), strides=(s, 1))[:] = True
        return m

    def guard_mask(self):
        """every output byte that no plane of any frame covers: it must still hold its initial content"""
        return ~self.covered("out")

    def fill_input(self, d_all, seed_base=0x360):
        """noise frames (fill_noise(frame_seed(f))) at the layout in a flat uint8 CUDA tensor of in_bytes; the bytes
        before frame 0 and after the last frame are noise too.  fill_noise stores 16 bytes at a time from a 16-byte
        aligned start: a frame that starts elsewhere is generated aside and copied."""
        import torch

        from transform360_amd import handler as T
        assert d_all.numel() == self.in_bytes
        T.fill_noise(d_all, T.frame_seed(0xFFFF, seed_base ^ 0xA11))
        tmp = torch.empty(self.in_frame_bytes if self.n_frames > 1 else self.in_bytes, dtype=torch.uint8, device=d_all.device)
        for f in range(self.n_frames):
            a = self.in_base + f * self.in_frame_bytes
            b = min(a + self.in_frame_bytes, self.in_bytes) if self.n_frames > 1 else self.in_bytes
            T.fill_noise(tmp[:b - a], T.frame_seed(f, seed_base))
            d_all[a:b].copy_(tmp[:b - a])


def _pick_width(r, cls, lo, hi):
    if cls == "mult16":
        return 16 * int(r.integers(max(1, (lo + 15) // 16), hi // 16 + 1))
    if cls == "mult4":
        while True:
            w = 4 * int(r.integers(max(1, (lo + 3) // 4), hi // 4 + 1))
            if w % 16:
                return w
    return 2 * int(r.integers(lo // 2, (hi - 1) // 2 + 1)) + 1


def _pick_stride(r, cls, w):
    if cls == "tight":
        return w
    if cls == "odd_pad":
        return w + 2 * int(r.integers(0, 8)) + 1
    return (w + 15) // 16 * 16 + 16 * int(r.choice([0, 0, 1, 4]))


def _frame_stride(cls, extent, bump=0):
    if cls == "tight":
        return extent + bump
    if cls == "mult4":
        fb = (extent + 3) // 4 * 4 + 4 * bump
        return fb + 4 if fb % 16 == 0 else fb
    return (extent + 255) // 256 * 256 + 256 * bump


def _place(r, planes, side, align):
    """offsets of the planes inside one frame, in order, with gaps; returns the frame's extent"""
    cur = 0
    for p in planes:
        w, h, s = (p.in_w, p.in_h, p.in_stride) if side == "in" else (p.out_w, p.out_h, p.out_stride)
        cur += int(r.choice([0, 0, 1, 3, 64]))
        cur = (cur + align - 1) // align * align
        if side == "in":
            p.in_off = cur
        else:
            p.out_off = cur
        cur += (h - 1) * s + w
    return cur


def draw_layout(seed, n_frames=None, n_planes=None):
    """One batch: context, planes, descriptors, frame strides, frame count and base offsets (module docstring)."""
    from tests.test_gpu_fuzz import draw
    r = np.random.default_rng(0x1A7 * 1000003 + seed)
    ov = draw(70000 + seed)[0]
    n = int(n_frames if n_frames is not None else r.choice(FRAME_COUNTS, p=_FRAME_WEIGHTS / _FRAME_WEIGHTS.sum()))
    npl = int(n_planes if n_planes is not None else r.choice(PLANE_COUNTS, p=_PLANE_WEIGHTS / _PLANE_WEIGHTS.sum()))
    # one side in four (each) is laid out for the fast branches: a 16-byte friendly source for the DMA gather and the fused
    # low-pass, dword friendly output; the rest draws every class at random
    in_fast, out_fast = r.random() < 0.4, r.random() < 0.4
    many_maps = r.random() < 0.15
    map_of = [int(r.integers(0, 8)) if many_maps else (0 if k == 0 else int(r.choice([0, 1, 1]))) for k in range(npl)]
    # sizes per map: luma-like for maps 0 and 2-7, chroma-like for map 1; smaller when the batch is long or wide
    big = n * npl <= 24
    lim = (640, 320, 384, 256) if big else (320, 160, 192, 128)
    maps, wcls = {}, {}
    for idx in sorted(set(map_of)):
        d = 2 if idx == 1 else 1
        ci = "mult16" if in_fast else str(r.choice(WIDTH_CLASSES))
        co = str(r.choice(WIDTH_CLASSES))
        iw = _pick_width(r, ci, 48 // d, lim[0] // d)
        ow = _pick_width(r, co, 24 // d, lim[2] // d)
        ih = int(r.integers(24 // d, lim[1] // d + 1))
        oh = int(r.integers(16 // d, lim[3] // d + 1))
        maps[idx] = (iw, ih, ow, oh)
        wcls[idx] = (ci, co)
    planes = []
    for k in range(npl):
        iw, ih, ow, oh = maps[map_of[k]]
        si = "mult16" if in_fast else str(r.choice(STRIDE_CLASSES))
        so = str(r.choice(["tight", "mult16"] if out_fast else STRIDE_CLASSES))
        so_w = (ow + 3) // 4 * 4 if out_fast and so == "tight" else ow
        planes.append(Plane(map_of[k], iw, ih, ow, oh, _pick_stride(r, si, iw), _pick_stride(r, so, so_w)))
    in_align = int(r.choice([16, 256])) if in_fast else int(r.choice([1, 1, 4, 16]))
    out_align = int(r.choice([4, 16, 256])) if out_fast else int(r.choice([1, 1, 4, 16]))
    ext_in, ext_out = _place(r, planes, "in", in_align), _place(r, planes, "out", out_align)
    fc_in = "mult256" if in_fast else str(r.choice(FRAME_CLASSES))
    fc_out = str(r.choice(["mult4", "mult256"])) if out_fast else str(r.choice(FRAME_CLASSES))
    ifb = _frame_stride(fc_in, ext_in)
    ofb = _frame_stride(fc_out, ext_out)
    if ofb == ifb:
        ofb = _frame_stride(fc_out, ext_out, 1)
    in_base = 0 if in_fast else int(r.choice(BASE_CLASSES))
    out_base = int(r.choice([0, 4, 8])) if out_fast else int(r.choice(BASE_CLASSES))
    L = Layout(seed=seed, ov=ov, planes=planes, maps=maps, n_frames=n, in_frame_bytes=ifb, out_frame_bytes=ofb,
               in_base=in_base, out_base=out_base,
               in_bytes=in_base + (n - 1) * ifb + ext_in + SLACK, out_bytes=out_base + (n - 1) * ofb + ext_out + SLACK)
    L.classes = dict(in_fast=in_fast, out_fast=out_fast, frame_in=fc_in, frame_out=fc_out, widths=wcls)
    return L


# ---- classification (what the generator's coverage test counts) ----
def stride_class(stride, w):
    if stride == w:
        return "tight"
    if stride % 16 == 0:
        return "mult16"
    if (stride - w) % 2 == 1 and stride - w <= 15:
        return "odd_pad"
    return "other"


def width_class(w):
    return "mult16" if w % 16 == 0 else "mult4" if w % 4 == 0 else "odd" if w % 2 else "other"


def frame_class(fb, extent):
    if fb % 256 == 0:
        return "mult256"
    if fb % 4 == 0 and fb % 16:
        return "mult4"
    if fb == extent:
        return "tight"
    return "other"


def extent(L, side):
    ps = L.planes
    if side == "in":
        return max(p.in_off + (p.in_h - 1) * p.in_stride + p.in_w for p in ps)
    return max(p.out_off + (p.out_h - 1) * p.out_stride + p.out_w for p in ps)


# ---- device helpers ----
def alloc(L):
    """(input, output) flat uint8 CUDA tensors of the layout's allocation sizes: noise in, SENTINEL out"""
    import torch
    d_in = torch.empty(L.in_bytes, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 256 == 0
    L.fill_input(d_in)
    d_out = torch.full((L.out_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_out.data_ptr() % 256 == 0
    torch.cuda.synchronize()
    return d_in, d_out


def handle(T, L, fused=False):
    import torch
    t = T.VideoFrameTransform(L.ctx())
    if fused:
        assert t.setFusedLowpass(True)  # before the maps
    for idx, d in L.maps.items():
        assert t.generateMapForPlane(*d, idx), (L.seed, idx, d)
    assert t.setStream(torch.cuda.current_stream())
    return t


def run_plain(t, L, d_in, d_out, pipelined=False):
    fn = t._l.T360_transformFramesPipelined if pipelined else t._l.T360_transformFrames
    descs = L.descs()
    return bool(fn(t._h, d_in.data_ptr() + L.in_base, L.in_frame_bytes, d_out.data_ptr() + L.out_base, L.out_frame_bytes,
                   L.n_frames, descs, len(descs)))


def run_posed(t, L, d_in, d_out, poses, in_frame_bytes=None):
    from transform360_amd import handler as T
    arr = T.make_poses(poses)
    assert len(arr) == L.n_frames
    descs = L.descs()
    ifb = L.in_frame_bytes if in_frame_bytes is None else in_frame_bytes
    return bool(t._l.T360_transformFramesPosed(t._h, d_in.data_ptr() + L.in_base, ifb, d_out.data_ptr() + L.out_base,
                                               L.out_frame_bytes, L.n_frames, descs, len(descs), arr))


def own_pose(L):
    ov = L.ov
    return (float(ov.get("fixed_yaw", 0.0)), float(ov.get("fixed_pitch", 0.0)), float(ov.get("fixed_roll", 0.0)))


def random_poses(L):
    r = np.random.default_rng(0x9053 + L.seed)
    return [(float(np.float32(r.uniform(-180, 180))), float(np.float32(r.uniform(-90, 90))), float(np.float32(r.uniform(-60, 60))))
            for _ in range(L.n_frames)]


def oracle_planes(O, ov, L, h_in, f, in_frame=None):
    """the planes of output frame f from an oracle handle of context `ov` (initial content SENTINEL)"""
    o = O.Oracle(filter_defaults(**ov), threads=ORACLE_THREADS)
    try:
        for idx, d in L.maps.items():
            assert o.generateMapForPlane(*d, idx)
        out = []
        for k, p in enumerate(L.planes):
            want = np.full((p.out_h, p.out_w), SENTINEL, np.uint8)
            src = np.ascontiguousarray(L.plane_view(h_in, f if in_frame is None else in_frame, k, "in"))
            assert o.transformFramePlane(src, want, p.map_idx, k)
            out.append(want)
        return out
    finally:
        o.close()


def check_oracle(O, L, h_in, h_out, frames=None, poses=None, in_frame=None):
    """the sampled frames' planes equal the oracle bit for bit; poses: one context per frame's pose"""
    base = None if poses is not None else oracle_handle(O, L)
    try:
        for f in (L.sample_frames() if frames is None else frames):
            if poses is None:
                wants = _planes_of(base, L, h_in, f if in_frame is None else in_frame)
            else:
                y, p, r = poses[f]
                wants = oracle_planes(O, dict(L.ov, fixed_yaw=y, fixed_pitch=p, fixed_roll=r), L, h_in, f, in_frame)
            for k, want in enumerate(wants):
                got = L.plane_view(h_out, f, k)
                bad = int((got != want).sum())
                assert bad == 0, "seed %d frame %d plane %d (map %d, %dx%d): %d px differ from the oracle" % (
                    L.seed, f, k, L.planes[k].map_idx, want.shape[1], want.shape[0], bad)
    finally:
        if base is not None:
            base.close()


def oracle_handle(O, L):
    o = O.Oracle(L.ctx(), threads=ORACLE_THREADS)
    for idx, d in L.maps.items():
        assert o.generateMapForPlane(*d, idx)
    return o


def _planes_of(o, L, h_in, fin):
    out = []
    for k, p in enumerate(L.planes):
        want = np.full((p.out_h, p.out_w), SENTINEL, np.uint8)
        assert o.transformFramePlane(np.ascontiguousarray(L.plane_view(h_in, fin, k, "in")), want, p.map_idx, k)
        out.append(want)
    return out


def check_guard(L, h_out, mask=None):
    m = L.guard_mask() if mask is None else mask
    bad = np.flatnonzero(h_out[m] != SENTINEL)
    if bad.size:
        where = np.flatnonzero(m)[bad[:4]]
        raise AssertionError("seed %d: %d bytes outside every plane changed (first at %s)" % (L.seed, bad.size, list(where)))
