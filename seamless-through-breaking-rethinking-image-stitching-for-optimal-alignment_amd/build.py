"""Build libstitch_gfx950.so (hipcc, gfx950 only) in-tree: ``python <pkg>/build.py``."""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libstitch_gfx950.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# geom.hip pins every fp32 rounding (bit-exact sample indices), inpaint.hip the Telea arrival times, tps_other.hip the fp64 remap
# maps, transref.hip the inpainter's pre / post steps, flow_splat.hip the warm start's fp64 nearest-source distances, multiband.hip every fp32 rounding of its pyramids,
# exposure.hip the fp64 gain solves and the fp32 smoothing / interpolation / apply chain, features.hip and features_ms.hip the fp64 RANSAC, dense_flow.hip the fp64 solve of every pixel: no fma contraction there (seam.hip, seam_gc.hip, crop.hip and patchmatch.hip are all integers)
SOURCES = {"gemm.hip": [], "gemm_split3.hip": [], "gemm_rows.hip": [], "nn.hip": [], "flowops.hip": [], "geom.hip": ["-ffp-contract=off"],
           "metrics.hip": ["-ffp-contract=off"], "operators.hip": [], "composition.hip": ["-ffp-contract=off"], "tps_pipeline.hip": ["-ffp-contract=off"], "patchembed.hip": [],
           "inpaint.hip": ["-ffp-contract=off"], "tps_other.hip": ["-ffp-contract=off"],
           "transref.hip": ["-ffp-contract=off"], "flow_splat.hip": ["-ffp-contract=off"], "jpeg.hip": [], "jpeg_dec.hip": [],
           "multiband.hip": ["-ffp-contract=off"], "exposure.hip": ["-ffp-contract=off"], "seam.hip": [], "seam_gc.hip": [], "crop.hip": [], "patchmatch.hip": [],
           "features.hip": ["-ffp-contract=off"], "dense_flow.hip": ["-ffp-contract=off"], "features_ms.hip": ["-ffp-contract=off"]}
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]
# No packed-fp32 VALU instructions (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32) anywhere in the library.  Measured in round 6
# (tools/neighbour_stress.py, profiles/r6_pk_f32_beside_bf16_mfma.txt): while another wave of the SIMD issues v_mfma_f32_32x32x16_bf16
# back to back (the split3 kernels, csrc/gemm_split3.h), a wave's v_pk_*_f32 results come back wrong in lanes 48-63 -- 80 % of the
# launches of the bilinear-resize kernel beside a split3 GEMM had corrupted 16-lane runs (DMA-only variant of the aggressor: none;
# MFMA-only: the same; the fp32-MFMA kernels as aggressor: none; torch's own elementwise kernels as victims: none).  The compiler's
# hazard tables cannot see another wave, so the instructions are simply not generated (scalar v_mul / v_add / v_fma instead).  NOT the same
# bits everywhere: under the default -ffp-contract a v_pk_mul_f32 + v_pk_add_f32 pair can come back as ONE scalar v_fma_f32, i.e. one rounding
# instead of two (the sources that pin their roundings carry -ffp-contract=off above).  Beside an MFMA stream the packed
# forms were the slower choice anyway -- MI355X_MICROARCH.md, packed f32 VALU.
COMMON += ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
if os.environ.get("ST_EXACT_TRANSCENDENTALS", "0") == "1":       # diagnostic build (csrc/common.h): not the shipped arithmetic
    COMMON.append("-DST_EXACT_TRANSCENDENTALS")


def compile_cmd(src, out, extra=()):
    """The command that compiles one of SOURCES (a file name in csrc/) to `out`: the library's flags, then `extra`, which says what to emit
    (build(): -c; tools/isa_waits.py: -S --cuda-device-only)."""
    return [HIPCC] + COMMON + SOURCES[src] + list(extra) + [os.path.join(CSRC, src), "-o", out]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    hdrs = [os.path.join(CSRC, "common.h"), os.path.join(CSRC, "gemm_common.h"), os.path.join(CSRC, "gemm_split3.h"), os.path.join(CSRC, "mlp_split3.h"), os.path.join(CSRC, "attn_small.h"),os.path.join(CSRC, "tps_solve.h"), os.path.join(CSRC, "jpeg_dec_core.h"), os.path.join(CSRC, "jpeg_tables.h"), os.path.join(CSRC, "jpeg_huff_core.h"), os.path.join(CSRC, "jpeg_scan.h"), os.path.join(CSRC, "jpeg_rst_core.h"), os.path.join(CSRC, "features_common.h"), os.path.join(HERE, "..", "include", "stitch_gfx950.h")]
    objs, jobs = [], []
    os.makedirs(os.path.join(CSRC, "_obj"), exist_ok=True)
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, "_obj", src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            jobs.append(compile_cmd(src, o, ["-c"]))
    if jobs:
        def run(cmd):
            if verbose:
                print(" ".join(cmd), flush=True)
            # (the HOST pass of a .hip file does not know the device-only target feature and says so once per pass: not a diagnostic of ours)
            r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
            err = "".join(l for l in r.stderr.splitlines(True) if "'-packed-fp32-ops' is not a recognized feature for this target" not in l)
            if err:
                sys.stderr.write(err)
            if r.returncode:
                raise subprocess.CalledProcessError(r.returncode, cmd)
        with ThreadPoolExecutor(max_workers=4) as ex:
            list(ex.map(run, jobs))
    if jobs or _stale(OUT, objs):
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
