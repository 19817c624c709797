"""Per-frame pose benchmark (T360_transformFramesPosed): BASELINE config 2 (3840x1920 yuv420p equirect -> 1536x1024
cubemap, bicubic, no low-pass), 64 frames per step, input rotating through a ring of frames several times the 256 MB
Infinity Cache (as bench.py does).  Prints one JSON line:

  posed               64 distinct poses per step: step ms, us per frame
  posed_static_pose   the same call with every pose equal to the context's
  transform_frames    T360_transformFrames on the same frames (the static path: map and LUT precomputed)
  regenerate          today's alternative without the feature: per pose a handle for that pose, generateMapForPlane x 2 and
                      one T360_transformFrames of one frame, synchronised (4 poses, ms per pose)
  regenerate_over_posed  regenerate ms per frame / posed ms per frame
  verified            2 frames of the last posed step, all planes, against the CPU oracle (bit-exact)

    python tools/bench_posed.py [--steps 20] [--warmup 3] [--out FILE]
"""
import argparse
import hashlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

IN_W, IN_H, OUT_W, OUT_H = 3840, 1920, 1536, 1024
FRAMES = 64
RING = 128  # 1.4 GB of input: every step reads its frames from HBM


def poses_for_step(k, n=FRAMES):
    """n distinct poses (a camera path: yaw sweeps the full circle, pitch and roll oscillate)"""
    return [(float(np.float32(-180.0 + 360.0 * (f + 0.5) / n + k)), float(np.float32(60.0 * math.sin(0.37 * f + k))),
             float(np.float32(10.0 * math.cos(0.91 * f)))) for f in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from transform360_amd import _lib, handler
    from transform360_amd.abi import CUBIC, filter_defaults
    if not torch.cuda.is_available():
        raise SystemExit("bench_posed.py needs a GPU")
    torch.cuda.set_device(0)
    ov = dict(interpolation_alg=CUBIC, enable_low_pass_filter=0)
    ctx = filter_defaults(**ov)
    lin, lout = handler.FrameLayout(IN_W, IN_H), handler.FrameLayout(OUT_W, OUT_H)
    d_in = torch.empty(RING * lin.frame_bytes, dtype=torch.uint8, device="cuda")
    for k in range(RING):
        handler.fill_noise(d_in[k * lin.frame_bytes:(k + 1) * lin.frame_bytes], handler.frame_seed(k))
    d_out = torch.zeros(FRAMES * lout.frame_bytes, dtype=torch.uint8, device="cuda")
    groups = RING // FRAMES
    stream = torch.cuda.current_stream()
    t = handler.VideoFrameTransform(ctx)
    for idx, k in ((0, 0), (1, 1)):
        assert t.generateMapForPlane(*lin.dims[k], *lout.dims[k], idx)
    assert t.setStream(stream)
    descs = t.plane_descs(lin, lout)
    L = t._l
    step_poses = [handler.make_poses(poses_for_step(k)) for k in range(groups)]
    still = handler.make_poses([(0.0, 0.0, 0.0)] * FRAMES)

    def src(k):
        return d_in.data_ptr() + (k % groups) * FRAMES * lin.frame_bytes

    def step_posed(k):
        assert L.T360_transformFramesPosed(t._h, src(k), lin.frame_bytes, d_out.data_ptr(), lout.frame_bytes, FRAMES, descs,
                                           len(descs), step_poses[k % groups])

    def step_still(k):
        assert L.T360_transformFramesPosed(t._h, src(k), lin.frame_bytes, d_out.data_ptr(), lout.frame_bytes, FRAMES, descs,
                                           len(descs), still)

    def step_static(k):
        assert L.T360_transformFrames(t._h, src(k), lin.frame_bytes, d_out.data_ptr(), lout.frame_bytes, FRAMES, descs,
                                      len(descs))

    def timed(step):
        for k in range(args.warmup):
            step(k)
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for k in range(args.steps):
                step(k)
            b.record(stream)
            b.synchronize()
            runs.append(a.elapsed_time(b) / args.steps)
        ms = sorted(runs)[len(runs) // 2]
        return {"step_ms": round(ms, 4), "us_per_frame": round(1000.0 * ms / FRAMES, 2),
                "runs_ms": [round(r, 4) for r in runs]}

    res = {"metric": "posed_config2_64_frames", "frames_per_step": FRAMES, "steps": args.steps, "repeats": args.repeats,
           "input_ring_frames": RING}
    res["transform_frames"] = timed(step_static)
    res["posed_static_pose"] = timed(step_still)
    res["posed"] = timed(step_posed)
    kernel = t.lastKernel()

    # the alternative without the feature: one handle + two maps per pose, one frame through it
    regen = []
    one = d_out[:lout.frame_bytes]
    for k, pose in enumerate(poses_for_step(0)[:5]):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c = filter_defaults(**dict(ov, fixed_yaw=pose[0], fixed_pitch=pose[1], fixed_roll=pose[2]))
        with handler.VideoFrameTransform(c) as h:
            for idx, p in ((0, 0), (1, 1)):
                assert h.generateMapForPlane(*lin.dims[p], *lout.dims[p], idx)
            assert h.setStream(stream)
            assert h.transformFrames(d_in[k * lin.frame_bytes:], lin.frame_bytes, one, lout.frame_bytes, 1,
                                     h.plane_descs(lin, lout))
            assert h.synchronize()
        if k > 0:  # the first one also pays the code-object loads of the map kernel
            regen.append(1000.0 * (time.perf_counter() - t0))
    res["regenerate"] = {"poses": len(regen), "ms_per_pose": round(sorted(regen)[len(regen) // 2], 3),
                         "runs_ms": [round(r, 3) for r in regen]}
    res["regenerate_over_posed"] = round(res["regenerate"]["ms_per_pose"] / (res["posed"]["step_ms"] / FRAMES), 1)

    # bit-exact check of frames 0 and 63 of one posed step against the oracle (outside the timed region)
    step_posed(0)
    torch.cuda.synchronize()
    from oracle import t360_oracle as O
    h_in = d_in[:FRAMES * lin.frame_bytes].cpu().numpy()
    h_out = d_out.cpu().numpy()
    poses = poses_for_step(0)
    bad = 0
    for f in (0, FRAMES - 1):
        o = O.Oracle(filter_defaults(**dict(ov, fixed_yaw=poses[f][0], fixed_pitch=poses[f][1], fixed_roll=poses[f][2])),
                     threads=8)
        for idx, p in ((0, 0), (1, 1)):
            assert o.generateMapForPlane(*lin.dims[p], *lout.dims[p], idx)
        fin = h_in[f * lin.frame_bytes:(f + 1) * lin.frame_bytes]
        fout = h_out[f * lout.frame_bytes:(f + 1) * lout.frame_bytes]
        for p in range(3):
            want = np.zeros((lout.dims[p][1], lout.dims[p][0]), np.uint8)
            assert o.transformFramePlane(lin.plane_view(fin, p), want, 1 if p else 0, p)
            bad += int((lout.plane_view(fout, p) != want).sum())
        o.close()
    res["verified"] = {"frames": [0, FRAMES - 1], "planes": 3, "differing_pixels": bad, "bit_exact": bad == 0}
    with open(_lib.LIB_PATH, "rb") as f:
        res["library_sha16"] = hashlib.sha256(f.read()).hexdigest()[:16]
    res["kernel"] = kernel
    res["device"] = torch.cuda.get_device_name(0)
    t.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
