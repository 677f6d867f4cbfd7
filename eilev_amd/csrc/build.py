"""Builds eilev_amd/csrc/libeilev_hip.so and its companions libeilev_hip_pld.so (prompt lookup), libeilev_hip_sample.so (device
sampling), libeilev_hip_rules.so (logits rules of greedy and beam search), libeilev_hip_t5beam.so (the flan-t5 decode step of beam search:
its own unit t5beam.o linked with the core library's objects, include/eilev_t5beam.h) and libeilev_hip_prefix.so (rows that continue one
shared prefix: prefix.o linked the same way, include/eilev_prefix.h) and libeilev_hip_kv8.so (the OPT decode step over an fp8 KV cache: kv8.o,
include/eilev_kv8.h) and libeilev_hip_w4.so (the OPT decode step over int4 weight-only linears: w4.o, include/eilev_w4.h) (gfx950) in-tree with hipcc.  Cross-compiles without a GPU."""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = ["gemm.hip", "gemm_pp4_ext.hip", "norm.hip", "attention.hip", "misc.hip", "attn_decode.hip", "vision.hip", "opt.hip", "t5.hip", "blocks.hip", "backward.hip", "comm.hip", "gemv.hip"]
HEADERS = ["common.h", "row_select.h", "stages.h", "gemm_common.h", "gemm_tiled.h", "gemm_pp4.h", "gemm_w6.h", "gemm_skinny.h", "attn_frame3.h", "attn_tile64.h", os.path.join("..", "..", "include", "eilev.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
         "-Wno-pass-failed"]
LIB = os.path.join(HERE, "libeilev_hip.so")
# The companion libraries: each its own source, public header and version script; none links the core library.  row_select.h is the device
# code that sample.hip and rules.hip share with misc.hip.
_INC = os.path.join("..", "..", "include")
COMPANIONS = [  # (source, headers, export map, output)
    ("pld.hip", ["common.h", os.path.join(_INC, "eilev.h"), os.path.join(_INC, "eilev_pld.h")], "exports_pld.map", "libeilev_hip_pld.so"),
    ("sample.hip", ["common.h", "row_select.h", os.path.join(_INC, "eilev.h"), os.path.join(_INC, "eilev_sample.h")], "exports_sample.map",
     "libeilev_hip_sample.so"),
    ("rules.hip", ["common.h", "row_select.h", os.path.join(_INC, "eilev.h"), os.path.join(_INC, "eilev_rules.h")], "exports_rules.map",
     "libeilev_hip_rules.so"),
]
# libeilev_hip_t5beam.so needs the decoder's GEMVs, norms and attention launchers: its one unit is linked with the core library's objects
# (no second compile of them); only eilev_t5beam_* is exported.  Not built for variants.
T5BEAM = ("t5beam.hip", [os.path.join(_INC, "eilev_t5beam.h")], "exports_t5beam.map", "libeilev_hip_t5beam.so")
# libeilev_hip_prefix.so: the same arrangement for prefix.hip (the OPT blocks around its own attention kernel); only eilev_prefix_* is exported
PREFIX = ("prefix.hip", [os.path.join(_INC, "eilev_prefix.h")], "exports_prefix.map", "libeilev_hip_prefix.so")
# libeilev_hip_kv8.so: the same arrangement for kv8.hip (the OPT decode step around its own fp8-cache attention kernel); only eilev_kv8_* is exported
KV8 = ("kv8.hip", [os.path.join(_INC, "eilev_kv8.h")], "exports_kv8.map", "libeilev_hip_kv8.so")
# libeilev_hip_w4.so: the same arrangement for w4.hip (the OPT decode step around its own int4 weight-streaming linear); only eilev_w4_* is exported
W4 = ("w4.hip", [os.path.join(_INC, "eilev_w4.h")], "exports_w4.map", "libeilev_hip_w4.so")
LINKED = (T5BEAM, PREFIX, KV8, W4)  # (source, headers, export map, output): one unit each, linked with the core library's objects


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    return "hipcc"


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_hip(force: bool = False, verbose: bool = False, variant: str = "", extra_flags=()) -> str:
    """``variant`` / ``extra_flags``: an A/B build of the same sources with extra -D flags into build/<variant>/ and
    libeilev_hip_<variant>.so (tools/gemm_ab.py compares two libraries in one process on one box)."""
    hdrs = [os.path.join(HERE, h) for h in HEADERS]
    objdir = os.path.join(HERE, "build", variant) if variant else os.path.join(HERE, "build")
    lib = os.path.join(HERE, f"libeilev_hip_{variant}.so") if variant else LIB
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    objs = []
    # (gemm.hip and gemm_pp4_ext.hip are by far the longest compiles — the persistent kernel's instances — and run side by side)
    units = [(src, src.replace(".hip", ".o"), []) for src in SOURCES]
    for src, obj, extra in units:
        s = os.path.join(HERE, src)
        o = os.path.join(objdir, obj)
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            jobs.append([_hipcc(), *FLAGS, *extra, *extra_flags, "-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        return r.stderr

    # the default build (no variant) also builds the companion libraries; the probe variant does not need them
    side_jobs = []
    for src, hdr, emap, out in COMPANIONS:
        src, emap, out = os.path.join(HERE, src), os.path.join(HERE, emap), os.path.join(HERE, out)
        if not variant and (force or _stale(out, [src, emap] + [os.path.join(HERE, h) for h in hdr])):
            side_jobs.append([_hipcc(), *FLAGS, *extra_flags, "-shared", "-o", out, src, "-Wl,--version-script=" + emap])

    linked = []  # (object, export map, library) of the companions that carry the core library's objects
    for src, hdr, emap, out in LINKED:
        l_src, l_obj = os.path.join(HERE, src), os.path.join(objdir, src.replace(".hip", ".o"))
        linked.append((l_obj, os.path.join(HERE, emap), os.path.join(HERE, out)))
        if not variant and (force or _stale(l_obj, [l_src] + hdrs + [os.path.join(HERE, h) for h in hdr])):
            jobs.append([_hipcc(), *FLAGS, *extra_flags, "-c", l_src, "-o", l_obj])

    with ThreadPoolExecutor(max_workers=len(SOURCES) + len(COMPANIONS) + len(LINKED)) as ex:
        side_futs = [ex.submit(run, j) for j in side_jobs]
        for warn in ex.map(run, jobs):
            if verbose and warn.strip():
                print(warn, file=sys.stderr)
        for fut in side_futs:
            warn = fut.result()
            if verbose and warn.strip():
                print(warn, file=sys.stderr)
    if force or jobs or _stale(lib, objs + [os.path.join(HERE, "exports.map")]):
        run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs, "-ldl", "-Wl,--version-script=" + os.path.join(HERE, "exports.map")])
    for l_obj, l_map, l_lib in linked:
        if not variant and (force or _stale(l_lib, objs + [l_obj, l_map])):
            run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", l_lib, l_obj, *objs, "-ldl", "-Wl,--version-script=" + l_map])
    return lib


if __name__ == "__main__":
    # python build.py [--force] [--variant NAME -DX=1 ...]
    args = [a for a in sys.argv[1:] if a != "--force"]
    name = ""
    if "--variant" in args:
        i = args.index("--variant")
        name = args[i + 1]
        del args[i:i + 2]
    print(build_hip(force="--force" in sys.argv, verbose=True, variant=name, extra_flags=tuple(args)))
