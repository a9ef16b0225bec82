"""Cases, inputs and the recording mode of tests/test_gpu_norm_bits.py: the GroupNorm and LayerNorm kernels of csrc/norm.hip held to the bits a
known-good commit wrote (tests/golden/norm_bits.json: the sha256 of every output's bytes).

Every input comes from integer arithmetic alone (no RNG, no library's float formulas), so the inputs are the same bytes everywhere.  GroupNorm
inputs are multiples of 1/4 with |x| <= 2 and at most 131072 elements per group: every partial sum (< 2^20 quarter steps) and sum of squares
(< 2^23 sixteenth steps) is exact in fp32, so the output bits depend on neither the chunking, the CU count nor which kernel folds the partials.
The two conv2d_gn cases normalise what the convolution wrote (not exact sums): their statistics arrive in the conv epilogue's fixed layout.
LayerNorm has no such dependence.

Recording (on the GPU, from a commit whose norm kernels are trusted - the fixture names the one it came from):
    python tests/norm_cases.py --commit <id of that commit> [--out tests/golden/norm_bits.json]
"""
import hashlib
import json
import os
import sys

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_bits.json")
NONE, SILU, RELU = 0, 1, 2

# (N, HW, C, act, with residual and accum through odise_hip_group_norm_ex); 32 groups
GN_CASES = [
    (2, 64, 320, SILU, False),       # few chunks: the apply kernel folds the partials
    (1, 8192, 128, NONE, False),     # 128 chunks on 256 CUs (> 64): gn_finalize_kernel runs
    (3, 256, 128, RELU, False),
    (1, 64, 2560, SILU, False),      # 320 vectors per pixel > 256: the v += VW loop of the statistics pass
    (1, 100, 512, NONE, False),      # ragged tail of the four-vector sweep
    (16, 64, 640, SILU, False),
    (1, 5, 96, NONE, False),         # 3 channels per group, fewer pixels than pixel lanes
    (2, 256, 256, RELU, True),
]
# (name, N, H, W, Cin, Cout, force_tile, force_split, eps, row blocks of statistics per image or None for "any"): both reach
# gn_finalize_cols_kernel.  The conv_in kernel only runs unforced (a forced tile or split keeps the implicit GEMM), so its case passes neither;
# its H * W / 256 row blocks show that it, and not the implicit GEMM, left the statistics.
CONV_CASES = [
    ("conv_gn_halo8_1x40x24x128x128", 1, 40, 24, 128, 128, 8, 1, 1e-6, None),
    ("conv_gn_conv_in_1x16x48", 1, 16, 48, 8, 128, -1, 0, 1e-6, 16 * 48 // 256),
]
# (rows, C, affine): one per instantiation of the LayerNorm kernel, plus ragged row counts at the thresholds 2048 and 32768
LN_CASES = [
    (9, 64, True), (100, 256, True),
    (2051, 256, True),               # four rows per half wave, ragged
    (77, 320, True), (2050, 512, True),
    (32771, 320, True),              # eight rows per wave
    (5, 768, True), (2049, 1024, True),
    (5, 1280, True), (2049, 2048, True),
    (3, 2560, True),                 # eight vectors per lane
    (100, 256, False),               # gamma = beta = NULL
]
# (rows, C, P) of the y2 = y + table[row % P] identity (no fixture)
TABLE_CASES = [(100, 256, 100), (2051, 256, 7), (33, 128, 33)]


def _ramp(n, mul, shift, mod, salt=0):
    """Integers in [0, mod): a 32-bit multiply-xorshift mix of the index (a bare multiply-and-shift repeats with a period of 8 elements, which
    would give every pixel of a GroupNorm input the same channel vector and hide a skipped pixel from the statistics)."""
    m32 = np.uint64(0xFFFFFFFF)
    h = ((np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(mul)) & m32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & m32
    h ^= h >> np.uint64(13)
    return ((h >> np.uint64(shift)) % np.uint64(mod)).astype(np.int64)


def quarters(shape, salt=0):
    """fp16 multiples of 1/4 in [-2, 2]."""
    n = int(np.prod(shape))
    return ((_ramp(n, 2654435761, 7, 17, salt) - 8) / 4.0).astype(np.float16).reshape(shape)


def weights(shape, salt=0):
    """fp16 multiples of 1/64 in [-1/8, 1/8] (convolution weights)."""
    n = int(np.prod(shape))
    return ((_ramp(n, 2246822519, 9, 17, salt) - 8) / 64.0).astype(np.float16).reshape(shape)


def gamma_beta(C):
    """fp32 gamma in [0.25, 1.75] (eighths), beta in [-5/16, 5/16] (sixteenths)."""
    return (((_ramp(C, 40503, 2, 13) - 6) / 8.0 + 1.0).astype(np.float32), ((_ramp(C, 9973, 1, 11) - 5) / 16.0).astype(np.float32))


def table(P, C):
    """fp32 [P, C] multiples of 1/32 in [-2, 2]."""
    return ((_ramp(P * C, 2654435761, 5, 129, 3) - 64) / 32.0).astype(np.float32).reshape(P, C)


def gn_name(N, HW, C, act, ex):
    return f"gn_{N}x{HW}x{C}_act{act}" + ("_res_accum" if ex else "")


def ln_name(rows, C, affine):
    return f"ln_{rows}x{C}" + ("" if affine else "_noaffine")


def run_gn(ctx, N, HW, C, act, ex):
    import ctypes
    x = ctx.to_device(quarters((N, HW, C)))
    g, b = (ctx.to_device(t) for t in gamma_beta(C))
    if not ex:
        return ctx.group_norm(x, g, b, 32, 1e-5, act).numpy()
    r, a = ctx.to_device(quarters((N, HW, C), salt=1 << 20)), ctx.to_device(quarters((N, HW, C), salt=1 << 21))
    y = ctx.empty((N, HW, C), np.float16)
    rc = ctx.lib.odise_hip_group_norm_ex(ctx.h, x.ptr, y.ptr, g.ptr, b.ptr, N, HW, C, 32, ctypes.c_float(1e-5), act, r.ptr, a.ptr)
    assert rc == 0, ctx.lib.odise_hip_last_error()
    return y.numpy()


def run_conv_gn(ctx, name, N, H, W, Cin, Cout, tile, split, eps, want_blocks):
    x = quarters((N, H, W, Cin))
    w = weights((Cout, 3, 3, Cin))
    if Cin == 8:   # the image convolution: three real channels, padded to eight with zeros
        x[..., 3:] = 0
        w[..., 3:] = 0
    g, b = gamma_beta(Cout)
    bias = ((_ramp(Cout, 7919, 1, 9) - 4) / 8.0).astype(np.float32)
    _, yn, blocks = ctx.conv2d_gn(ctx.to_device(x), ctx.to_device(w), ctx.to_device(g), ctx.to_device(b), bias=ctx.to_device(bias), eps=eps, act=SILU,
                                  force_tile=tile, force_split=split)
    assert blocks > 0, f"{name}: the convolution left no statistics (the stand-alone GroupNorm ran instead of gn_finalize_cols_kernel)"
    assert want_blocks is None or blocks == want_blocks, f"{name}: {blocks} row blocks of statistics, {want_blocks} expected from the kernel this case is about"
    return yn.numpy()


def ln_input(rows, C):
    return quarters((rows, C)) * np.float16(2) + np.float16(0.5)    # fp16 in [-3.5, 4.5], exact


def run_ln(ctx, rows, C, affine):
    g, b = (ctx.to_device(t) for t in gamma_beta(C)) if affine else (None, None)
    return ctx.layer_norm(ctx.to_device(ln_input(rows, C)), g, b, 1e-5).numpy()


def cases():
    """[(name, callable(ctx) -> numpy output)] in a fixed order."""
    out = [(gn_name(*c), lambda ctx, c=c: run_gn(ctx, *c)) for c in GN_CASES]
    out += [(c[0], lambda ctx, c=c: run_conv_gn(ctx, *c)) for c in CONV_CASES]
    out += [(ln_name(*c), lambda ctx, c=c: run_ln(ctx, *c)) for c in LN_CASES]
    return out


def digest(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load_fixture() -> dict:
    with open(FIXTURE) as f:
        return json.load(f)


def record(commit: str, out_path: str) -> dict:
    import subprocess
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from odise_amd.runtime import Context
    ctx = Context(0)
    try:
        hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()
        hipcc = next((l.strip() for l in hipcc if "HIP version" in l), hipcc[0].strip() if hipcc else "unknown")
    except OSError:
        hipcc = "unknown"
    # the runtime's name of the device: its marketing name (empty on some systems) and the architecture string in brackets; kept as reported
    rec = {"commit": commit, "device": ctx.device_info()[0].strip(), "cu_count": ctx.device_info()[1], "hipcc": hipcc,
           "cases": {name: digest(run(ctx)) for name, run in cases()}}
    ctx.close()
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return rec


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="record tests/golden/norm_bits.json from the built library (run on a commit whose norm kernels are trusted)")
    ap.add_argument("--commit", required=True, help="id of the commit the library was built from")
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    r = record(a.commit, a.out)
    print(f"{len(r['cases'])} cases from {r['commit']} on {r['device']} -> {a.out}")
