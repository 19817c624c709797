"""Build tests/c/_build/vf_harness: the reference's UNMODIFIED ffmpeg filter (Transform360/vf_transform360.c, compiled
against the test-only libav stand-ins in tests/c/avstub into oracle/_ref/vf_transform360.o by `make -C oracle ref`)
+ tests/c/vf_harness.c, linked against libTransform360.so the way ffmpeg's --extra-libs='-lTransform360 -lstdc++' does.

Where the reference sources are absent the filter OBJECT of oracle/_ref (git-ignored, like the rest of the reference
build) is what the harness links; the reference source is never copied."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
BUILD = os.path.join(HERE, "_build")
FILTER_OBJ = os.path.join(ROOT, "oracle", "_ref", "vf_transform360.o")
HARNESS = os.path.join(BUILD, "vf_harness")


def build(lib_path):
    """Returns the harness path, or None when the reference build has no filter object."""
    if not os.path.exists(FILTER_OBJ):
        return None
    os.makedirs(BUILD, exist_ok=True)
    common = ["gcc", "-std=gnu11", "-O1", "-w", "-I", os.path.join(HERE, "avstub"), "-I", os.path.join(ROOT, "include")]
    hobj = os.path.join(BUILD, "vf_harness.o")
    subprocess.check_call(common + ["-c", os.path.join(HERE, "vf_harness.c"), "-o", hobj])
    libdir = os.path.dirname(lib_path)
    subprocess.check_call(["gcc", "-o", HARNESS, hobj, FILTER_OBJ, "-L", libdir, "-lTransform360", "-lstdc++", "-lm",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return HARNESS
