"""Case tables and helpers of tests/test_classical_reject_cpu.py and tests/test_classical_matrix_gpu.py: what protects the kernels of
csrc/features.hip, features_ms.hip, dense_flow.hip, patchmatch.hip, seam_gc.hip and crop.hip from a call outside their contract.

Part A, the refusal matrix.  The operand list of every `st_*` entry of the six files is parsed from include/stitch_gfx950.h (never from
the region tables of the .hip files, so an operand that a region table forgot shows up as a case that is not refused): a `const T*` is an
input, `workspace` the workspace, a `*_host` pointer host memory, every other pointer an output.  For each entry BASE holds one record the
contract accepts (scalars, and `Ptr(operand, delta)` for a pointer: the start of that operand plus delta bytes); `table()` derives every
variant from it by replacing exactly one field (`_vary` asserts that).  A variant is refused ("refuse": the entry's refusal code, ST_EINVAL
or, for the size helpers, 0) or accepted ("accept").  Accepted rows of the entries that launch are: an optional pointer given as null with
its channel count left nonzero, and one input starting where another input starts; each names the `equal` call, the base on other
contents, that must give the same bits.  The limits B, H, W of the entries that launch are exercised as accepted calls by part C of the
GPU file; the host-only helpers take their accepted rows at each limit right here.

Parts B and C: the device-side guards restated (`describe_guarded`, `ms_describe_guarded`, `ransac_guarded`, `ms_ransac_guarded`), the
saturated images and the scenes of the corner cases.  The restatements form every sum in int64 (numpy) or Python ints: `luma`, `sobel`,
`harris`, `window_sum` of tests/_features_ref.py and `gradients`, `sample`, `window_sum`, `solve` of tests/_dense_flow_ref.py work on int64
arrays throughout, which is what makes a comparison with them an independent check of the kernels' int and int16 arithmetic.

Nothing here needs a GPU to import; `table()` loads the library for the workspace sizes (host arithmetic)."""
import collections
import ctypes as C
import functools
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stitch_gfx950.h")
EINVAL = 1001
PREFIXES = ("st_feature_", "st_dense_flow", "st_seam_gc_", "st_inner_rect", "st_patchmatch_")
_CTYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}

Ptr = collections.namedtuple("Ptr", "operand delta")
Arg = collections.namedtuple("Arg", "name ctype role")                # role: scalar, in, out, ws, host, stream
Case = collections.namedtuple("Case", "entry field value kind expect equal")


# ---- the header's operand lists ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def entries():
    """{entry: [Arg]} for every `int st_*(...)` of the six files, in the header's order"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(st_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S):
        if not m.group(1).startswith(PREFIXES):
            continue
        args = []
        for a in m.group(2).split(","):
            words = " ".join(a.replace("*", " * ").split()).split(" ")
            name, ptr, const = words[-1], "*" in words, words[0] == "const"
            if not ptr:
                role, ctype = "scalar", _CTYPES[words[0]]
            else:
                ctype = C.c_void_p
                role = "stream" if name == "stream" else "host" if name.endswith("_host") else "ws" if name == "workspace" else "in" if const else "out"
            args.append(Arg(name, ctype, role))
        out[m.group(1)] = args
    return out


def family(entry):
    return ("ms" if entry.startswith("st_feature_ms_") else "ft" if entry.startswith("st_feature_") else "df" if entry.startswith("st_dense_flow") else
            "gc" if entry.startswith("st_seam_gc_") else "cr" if entry.startswith("st_inner_rect") else "pm")


# ---- the contract's ranges (include/stitch_gfx950.h) ---------------------------------------------------------------------------------------------
_FT = dict(B=(1, 64), H=(64, 1024), W=(64, 1024), max_hyp=(1, 65536), min_inliers=(0, None), levels=(1, 8), oriented=(0, 1))
LIMITS = dict(ft=_FT, ms=_FT, df=dict(B=(1, 64), H=(16, 1024), W=(16, 1024), levels=(1, 8), iters=(1, 16), radius=(1, 7), damping=(0, 1 << 24)),
              gc=dict(H=(1, 4096), W=(1, 4096)), cr=dict(H=(1, 4096), W=(1, 4096)), pm=dict(H=(15, 4096), W=(15, 4096), levels=(0, 8), iters=(0, 64)))
THR_REFUSED = (0.0, -1.0, float("nan"), float("inf"))
CHANNELS_REFUSED = (0, 2, 4)
OPTIONAL = {("st_dense_flow_pyramid", "mask1"), ("st_dense_flow_pyramid", "mask2"), ("st_dense_flow", "mask1"), ("st_dense_flow", "mask2"),
            ("st_inner_rect", "mask2"), ("st_inner_rect", "runs_out"), ("st_patchmatch_fill", "nnf_out"), ("st_patchmatch_fill", "sad_out"),
            ("st_feature_ms_level_sizes", "sizes_host")}
# an entry that launches nothing refuses with 0 where its comment in the header says so
REFUSAL = {"st_feature_slots": 0, "st_feature_workspace_bytes": 0, "st_feature_ms_level_sizes": 0, "st_feature_ms_slots": 0, "st_feature_ms_workspace_bytes": 0,
           "st_seam_gc_workspace_bytes": 0, "st_inner_rect_workspace_bytes": 0, "st_patchmatch_levels": 0, "st_patchmatch_workspace_bytes": 0}
HOST_ONLY = set(REFUSAL) | {"st_feature_brief_pattern", "st_feature_workspace_layout", "st_feature_ms_workspace_layout", "st_dense_flow_workspace_bytes",
                            "st_dense_flow_workspace_layout"}


def no_refusal(entry):
    """the fields of an entry that no value of theirs alone makes it refuse: the seed, the stream, a host pointer that may be null"""
    return {a.name for a in entries()[entry] if a.name in ("seed", "stream") or (a.role == "host" and (entry, a.name) in OPTIONAL)}


# ---- base records ------------------------------------------------------------------------------------------------------------------------------
_SCALARS = dict(ft=dict(B=2, H=65, W=97, max_hyp=100, thr=3.0, min_inliers=6, seed=1),
                ms=dict(B=2, H=96, W=128, levels=2, oriented=1, max_hyp=100, thr=3.0, min_inliers=6, seed=1),
                df=dict(B=2, H=33, W=65, levels=2, iters=2, radius=2, damping=65536, mask1_channels=1, mask2_channels=3),
                gc=dict(H=20, W=40), cr=dict(H=20, W=40), pm=dict(H=24, W=40, levels=2, iters=2, seed=1))


def ft_slots(H, W):
    return 4 * -(-H // 32) * -(-W // 32)


def ms_level_sizes(H, W, levels):
    out = [(H, W)]
    while len(out) < min(levels, 8) and min(4 * out[-1][0] // 5, 4 * out[-1][1] // 5) >= 64:
        out.append((4 * out[-1][0] // 5, 4 * out[-1][1] // 5))
    return out


def _need(entry, a):
    """workspace_bytes the entry needs for the (accepted) scalars a"""
    from stitch_amd._lib import lib
    if entry in ("st_feature_ransac", "st_feature_ms_ransac"):
        N = ft_slots(a["H"], a["W"]) if entry == "st_feature_ransac" else sum(ft_slots(h, w) for h, w in ms_level_sizes(a["H"], a["W"], a["levels"]))
        return 32 * a["B"] * N + 4 * a["B"] * a["max_hyp"]
    if entry == "st_dense_flow_iterate":
        return 8 * a["B"] * a["H"] * a["W"]
    if entry == "st_feature_homography":
        return lib.st_feature_workspace_bytes(a["B"], a["H"], a["W"], a["max_hyp"])
    if entry == "st_feature_ms_homography":
        return lib.st_feature_ms_workspace_bytes(a["B"], a["H"], a["W"], a["levels"], a["max_hyp"])
    if entry in ("st_dense_flow", "st_dense_flow_pyramid"):
        n = C.c_int64(0)
        assert lib.st_dense_flow_workspace_bytes(a["B"], a["H"], a["W"], a["levels"], C.cast(C.byref(n), C.c_void_p)) == 0
        return int(n.value)
    if entry.startswith("st_seam_gc_"):
        return lib.st_seam_gc_workspace_bytes(a["H"], a["W"])
    if entry == "st_inner_rect":
        return lib.st_inner_rect_workspace_bytes(a["H"], a["W"])
    if entry == "st_patchmatch_fill":
        return lib.st_patchmatch_workspace_bytes(a["H"], a["W"], a["levels"])
    raise KeyError(entry)


def sizes(entry, a):
    """{device operand: bytes} by the header's shapes, for any integers a (a refused shape included); the workspace is not in it"""
    g = lambda k: max(int(a.get(k, 1)), 0)                                                         # noqa: E731
    B, H, W = g("B"), g("H"), g("W")
    px, n, fam = B * H * W, H * W, family(entry)
    if fam == "ft":
        N, P = ft_slots(H, W), H * W
    elif fam == "ms":
        lv = ms_level_sizes(H, W, max(g("levels"), 1))
        N, P = sum(ft_slots(h, w) for h, w in lv), sum(h * w for h, w in lv)
    bn = B * N if fam in ("ft", "ms") else 0
    stage = dict(kp1=8 * bn, kp2=8 * bn, desc1=32 * bn, desc2=32 * bn, nn_out=24 * bn, matches_out=8 * bn, count_out=4 * B, matches=8 * bn, count=4 * B,
                 motion_out=32 * B, H_out=36 * B, info_out=32 * B, mask_out=bn, xy_out=32 * bn, img1=12 * px, img2=12 * px)
    full = {
        "st_feature_detect": dict(img=12 * px, kp_out=8 * bn, box_out=2 * px),
        "st_feature_describe": dict(box=2 * px, kp=8 * bn, desc_out=32 * bn),
        "st_feature_ms_pyramid": lambda: dict(img=12 * px, pyr_out=B * P),
        "st_feature_ms_detect": lambda: dict(pyr=B * P, kp_out=8 * bn, bins_out=bn, box_out=2 * B * P),
        "st_feature_ms_describe": lambda: dict(box=2 * B * P, kp=8 * bn, bins=bn, desc_out=32 * bn),
        "st_dense_flow_iterate": dict(v1=2 * px, v2=2 * px, m1=px, m2=px, u=8 * px, u_out=8 * px, support_out=px),
        "st_seam_gc_begin": dict(img1=12 * n, img2=12 * n, mask1=4 * n, mask2=4 * n),
        "st_seam_gc_finish": dict(side_out=n, info_out=16),
        "st_inner_rect": dict(mask1=4 * n, mask2=4 * n, info_out=24, runs_out=2 * n),
        "st_patchmatch_fill": dict(img=3 * n, mask=n, out=3 * n, info_out=16, nnf_out=8 * n, sad_out=4 * n),
    }.get(entry)
    if callable(full):
        full = full()
    if full is None:
        if fam == "df":
            full = dict(img1=12 * px, img2=12 * px, mask1=4 * g("mask1_channels") * px, mask2=4 * g("mask2_channels") * px, flow_out=8 * px, support_out=px)
        else:
            full = stage
    return {x.name: full[x.name] for x in entries()[entry] if x.role in ("in", "out")}


@functools.lru_cache(maxsize=None)
def base(entry):
    """the accepted record of an entry: {field: value}; a pointer is Ptr(its own operand, 0), the stream None"""
    rec, sc = {}, _SCALARS[family(entry)]
    for a in entries()[entry]:
        if a.role == "scalar" and a.name != "workspace_bytes":
            rec[a.name] = sc[a.name]
        elif a.role == "stream":
            rec[a.name] = None
        elif a.role != "scalar":
            rec[a.name] = Ptr(a.name, 0)
    if "workspace_bytes" in [a.name for a in entries()[entry]]:
        rec["workspace_bytes"] = _need(entry, rec)
    return rec


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def _vary(entry, field, value, kind, expect="refuse", equal=None):
    b = base(entry)
    rec = dict(b, **{field: value})
    assert field in b and sum(not _same(rec[k], b[k]) for k in b) == 1 and set(rec) == set(b), (entry, field, value)
    return Case(entry, field, value, kind, expect, equal)


def record(case):
    return dict(base(case.entry), **{case.field: case.value})


def pairs(entry):
    """the unordered (output, other) pairs of device operands the header's list forms, the workspace being an output"""
    ops = [a for a in entries()[entry] if a.role in ("in", "out", "ws")]
    return [(x.name, y.name) for i, x in enumerate(ops) for y in ops[i + 1:] if x.role != "in" or y.role != "in"]


@functools.lru_cache(maxsize=None)
def table():
    """every Case of every entry"""
    out = []
    for entry, args in entries().items():
        b, lim, names = base(entry), LIMITS[family(entry)], [a.name for a in args]
        size = dict(sizes(entry, b), **({"workspace": b["workspace_bytes"]} if "workspace" in names else {}))
        role = {a.name: a.role for a in args}
        for a in args:
            f = a.name
            if a.role == "scalar" and f in lim:
                lo, hi = lim[f]
                out.append(_vary(entry, f, lo - 1, "below"))
                if hi is not None:
                    out.append(_vary(entry, f, hi + 1, "above"))
                if entry in HOST_ONLY:
                    out += [_vary(entry, f, v, "at_limit", "accept") for v in (lo, hi) if v is not None and v != b[f]]
            elif f == "thr":
                out += [_vary(entry, f, v, "param") for v in THR_REFUSED]
            elif f.endswith("_channels"):
                out += [_vary(entry, f, v, "param") for v in CHANNELS_REFUSED]
            elif f == "workspace_bytes":
                out.append(_vary(entry, f, b[f] - 1, "short"))
            elif a.role == "ws":
                out += [_vary(entry, f, None, "null"), _vary(entry, f, Ptr(f, 4), "misaligned4"), _vary(entry, f, Ptr(f, 8), "misaligned8")]
            elif a.role in ("in", "out", "host"):
                if (entry, f) in OPTIONAL:
                    eq = {"mask1": ("ones", f), "mask2": ("zeros" if entry == "st_inner_rect" else "ones", f)}.get(f)
                    out.append(_vary(entry, f, None, "null_optional", "accept", eq))
                else:
                    out.append(_vary(entry, f, None, "null"))
        # an output against every other operand: it starts on the other's last byte, the other starts on its last byte, the two start together.
        # The workspace has to stay aligned, so against it the other operand is the one that moves.
        for x, y in pairs(entry):
            if role[x] == "ws":
                x, y = y, x
            out.append(_vary(entry, x, Ptr(y, size[y] - 1), f"overlap:{x}|{y}:first_on_last"))
            if role[y] == "ws":
                out.append(_vary(entry, x, Ptr(y, 1 - size[x]), f"overlap:{x}|{y}:last_on_first"))
            else:
                out.append(_vary(entry, y, Ptr(x, size[x] - 1), f"overlap:{x}|{y}:last_on_first"))
            out.append(_vary(entry, x, Ptr(y, 0), f"overlap:{x}|{y}:equal"))
        # an input that starts where another input starts is accepted: the smaller one moves, and the call equals the base with the moved
        # operand's contents replaced by the bytes it now reads
        ins = [a.name for a in args if a.role == "in"]
        for i, x in enumerate(ins):
            for y in ins[i + 1:]:
                small, big = (x, y) if size[x] <= size[y] else (y, x)
                out.append(_vary(entry, small, Ptr(big, 0), f"alias:{small}={big}", "accept", ("copy", small, big)))
    return out


def refusals(entry=None):
    return [c for c in table() if c.expect == "refuse" and (entry is None or c.entry == entry)]


def accepted(entry=None):
    return [c for c in table() if c.expect == "accept" and (entry is None or c.entry == entry)]


def case_id(c):
    v = c.value
    return f"{c.entry[3:]}-{c.field}-{c.kind}" + ("" if isinstance(v, Ptr) or v is None or c.kind in ("short",) else f"-{v}")


def call(entry, rec, address):
    """the entry on a record; `address(operand)` gives the start of a device or host operand"""
    from stitch_amd._lib import lib
    argv = []
    for a in entries()[entry]:
        v = rec[a.name]
        if a.role == "scalar":
            argv.append(a.ctype(v))
        elif v is None:
            argv.append(None)
        else:
            argv.append(C.c_void_p(address(v.operand) + v.delta))
    return int(getattr(lib, entry)(*argv))


# ---- part B: the device-side guards, restated -------------------------------------------------------------------------------------------------
import _features_ms_ref as msref  # noqa: E402
import _features_ref as ftref  # noqa: E402

I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def describe_guarded(box, kp):
    """_features_ref.describe under ft_describe_kernel's guard: a keypoint outside border <= x < W - border, border <= y < H - border reads
    nothing and gives a zero descriptor"""
    H, W = box.shape
    ok = (kp[:, 0] >= ftref.BORDER) & (kp[:, 0] < W - ftref.BORDER) & (kp[:, 1] >= ftref.BORDER) & (kp[:, 1] < H - ftref.BORDER)
    return ftref.describe(box, np.where(ok[:, None], kp, -1).astype(np.int32))


def ms_describe_guarded(boxes, kp, bins, H, W, levels):
    """_features_ms_ref.describe_level per level under ftms_describe_kernel's guards: the border test against the slot's own level, bins & 31"""
    starts, out = msref.slot_starts(H, W, levels), []
    for l, box in enumerate(boxes):
        k, b = kp[starts[l]:starts[l + 1]], bins[starts[l]:starts[l + 1]].astype(np.int64) & 31
        h, w = box.shape
        ok = (k[:, 0] >= msref.BORDER) & (k[:, 0] < w - msref.BORDER) & (k[:, 1] >= msref.BORDER) & (k[:, 1] < h - msref.BORDER)
        out.append(msref.describe_level(box, np.where(ok[:, None], k, -1).astype(np.int32), b * ok))
    return np.concatenate(out)


def clamp_list(matches, count, N, clamp=True):
    """ft_count and ft_norm_kernel's index rule: count to 0..N, every index of the list to 0..N-1.  clamp=False drops the index rule (what
    the mutation check of the pull request plants): an index then wraps the way numpy indexing does"""
    m = int(min(max(int(count), 0), N))
    mt = np.asarray(matches, np.int64)
    return (np.clip(mt, 0, N - 1) if clamp else mt).astype(np.int64), m


def ransac_guarded(kp1, kp2, matches, count, H, W, clamp=True, **kw):
    mt, m = clamp_list(matches, count, len(kp1), clamp)
    return ftref.ransac(kp1, kp2, mt, m, H, W, **kw)


def ms_ransac_guarded(kp1, kp2, matches, count, H, W, levels, clamp=True, **kw):
    mt, m = clamp_list(matches, count, min(len(kp1), 11520), clamp)                    # (ftms_refit_kernel: FTMS_MAX_SLOTS, never below N)
    return msref.ransac(kp1, kp2, mt, m, H, W, levels, **kw)


HOSTILE_COUNTS = ("-5", "0", "7", "8", "N", "N+1", "i32max")
HOSTILE_INDICES = (-1, "N", I32_MAX, I32_MIN)


def planted_list(H, W, n=24):
    """_features_ref.planted_matches("outliers") for any accepted size: n points under a homography, every third displaced by 8..19 px
    -> (kp1, kp2 int32 [N,2], matches int32 [N,2], n)"""
    N, rng = ftref.slots(H, W), np.random.default_rng(21)
    Hm = ftref.homography_matrix(H, W, 5, -3, 2.0, 1e-4, -5e-5)
    p = np.stack([rng.choice(np.arange(16, W - 16), n, replace=False), rng.choice(np.arange(16, H - 16), n, replace=False)], 1)
    q = np.c_[p, np.ones(n)] @ Hm.T
    q = np.rint(q[:, :2] / q[:, 2:]).astype(np.int64)
    q[::3] += rng.integers(8, 20, (len(q[::3]), 2))
    q = np.clip(q, 0, [W - 1, H - 1])
    kp1, kp2 = np.full((N, 2), -1, np.int32), np.full((N, 2), -1, np.int32)
    s1, s2 = np.sort(rng.choice(N, n, replace=False)), rng.choice(N, n, replace=False)
    kp1[s1], kp2[s2] = p, q
    matches = np.full((N, 2), -1, np.int32)
    matches[:n] = np.stack([s1, s2], 1)
    return kp1, kp2, matches, n


def hostile_matches(H, W, bad):
    """planted_list with the index `bad` planted inside the list, in place of the slots of two inliers (entry 4,
    image 1; entry 5, image 2).  Slot N - 1, where a wrapped -1 lands, holds those inliers' own keypoints and slot 0, where the clamp lands,
    a far one: the clamp costs two inliers, so the two rules give different bits -> (kp1, kp2, matches int32 [N,2], m)"""
    kp1, kp2, matches, m = planted_list(H, W)
    N = len(kp1)
    for col, kp in ((0, kp1), (1, kp2)):                                            # the list leaves slots 0 and N - 1 alone
        for s in (0, N - 1):
            if s in matches[:m, col]:
                t = next(t for t in range(1, N - 1) if t not in matches[:m, col])
                kp[t], matches[:m, col] = kp[s], np.where(matches[:m, col] == s, t, matches[:m, col])
    kp1[N - 1], kp2[N - 1] = kp1[matches[4, 0]], kp2[matches[5, 1]]
    kp1[0], kp2[0] = (W - 17, 16), (16, H - 17)
    matches[4, 0] = matches[5, 1] = N if bad == "N" else bad
    return kp1, kp2, matches, m


def hostile_count(name, N):
    return {"-5": -5, "0": 0, "7": 7, "8": 8, "N": N, "N+1": N + 1, "i32max": I32_MAX}[name]


def hostile_keypoints(H, W, border, N):
    """int32 [N,2]: the corner and border cases of the issue in the first slots, (-1, -1) behind them"""
    pts = [(-1, -1), (0, 0), (W - 1, H - 1), (W, H), (I32_MAX, I32_MAX), (I32_MIN, 5), (border - 1, border), (border, border - 1), (border, border),
           (W - border, border), (W - border - 1, border), (border, H - border), (border, H - border - 1), (W - border - 1, H - border - 1),
           (W // 2, H // 2), (5, I32_MIN), (W // 2, I32_MAX)]
    kp = np.full((N, 2), -1, np.int64)
    kp[:len(pts)] = pts
    return kp.astype(np.int32)


# flow: 256 x + u must stay inside int32 for x <= 1023, and u + du (|du| <= 256) too: |u| <= 2^31 - 1 - 256 * 1023 - 256
FLOW_U_BOUND = I32_MAX - 256 * 1023 - 256
HOSTILE_U = (1 << 20, -(1 << 20), I32_MAX // 2, -(I32_MAX // 2), FLOW_U_BOUND, -FLOW_U_BOUND)


def hostile_flow(H, W, seed=3):
    """int64 [2,H,W]: the hostile magnitudes scattered over a small random field, and rows / columns whose sample position is exactly -1, 0,
    W - 2, W - 1 (x) and -1, 0, H - 2, H - 1 (y)"""
    rng = np.random.default_rng(seed)
    U = rng.integers(-600, 600, (2, H, W)).astype(np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    for k, v in enumerate(HOSTILE_U):
        U[k % 2, (3 * k + 1) % H, (5 * k + 2) % W] = v
        U[(k + 1) % 2, (7 * k + 4) % H, (11 * k + 3) % W] = v
    for r, target in enumerate((-1, 0, W - 2, W - 1)):
        U[0, 4 + r] = 256 * (target - xs[4 + r])
    for c, target in enumerate((-1, 0, H - 2, H - 1)):
        U[1, :, 9 + c] = 256 * (target - ys[:, 9 + c])
    return U


# ---- part C: saturated images --------------------------------------------------------------------------------------------------------------------
SATURATED = ("checker", "steps", "steps_swapped", "nonfinite")


def saturated_pair(name, H=96, W=128):
    """img1, img2 fp32 [1,3,H,W]: a one-pixel 0 / 255 checkerboard against its one-pixel shift; 0 / 255 vertical steps of period 2 against
    period 3, and the two swapped (the central difference of period 2 is zero away from the border, that of period 3 is not); a scene
    with +Inf / -Inf / 1e30 / -1e30 planted where _features_ref.degenerate("nonfinite") plants its values"""
    ys, xs = np.mgrid[0:H, 0:W]
    g = lambda p: np.ascontiguousarray(np.broadcast_to(p.astype(np.float32), (1, 3, H, W)))       # noqa: E731
    if name == "checker":
        return g(255 * ((ys + xs) % 2)), g(255 * ((ys + xs + 1) % 2))
    if name in ("steps", "steps_swapped"):
        p2, p3 = g(255 * (xs % 2)), g(255 * (xs % 3 == 0))
        return (p2, p3) if name == "steps" else (p3, p2)
    a, b = (t.copy() for t in ftref.small_pair(H, W))
    rng = np.random.default_rng(11)
    for img in (a, b):
        flat = img.reshape(-1)
        idx = rng.choice(flat.size, 400, replace=False)
        flat[idx[:100]], flat[idx[100:200]], flat[idx[200:300]], flat[idx[300:]] = np.inf, -np.inf, 1e30, -1e30
    return a, b


def cycled(items, times):
    """[B,...] from `items` repeated `times` times in order"""
    return np.ascontiguousarray(np.concatenate([np.concatenate(items)] * times))


# ---- part A on live buffers: what the base record of every entry that launches reads, and what it must write -----------------------------------
import _crop_ref as crref  # noqa: E402
import _dense_flow_ref as dfref  # noqa: E402
import _patchmatch_ref as pmref  # noqa: E402
import _seam_gc_ref as gcref  # noqa: E402


def feature_items(H, W):
    """img1, img2 fp32 [2,3,H,W]: a pair with a large overlap, then an identical pair"""
    p, q = ftref.small_pair(H, W), ftref.degenerate("identical", H, W)
    return np.concatenate([p[0], q[0]]), np.concatenate([p[1], q[1]])


@functools.lru_cache(maxsize=None)
def _ft_want():
    s = _SCALARS["ft"]
    a, b = feature_items(s["H"], s["W"])
    return a, b, ftref.homography(a, b, max_hyp=s["max_hyp"], thr=s["thr"], min_inliers=s["min_inliers"], seed=s["seed"])


@functools.lru_cache(maxsize=None)
def _ms_want():
    s = _SCALARS["ms"]
    a, b = feature_items(s["H"], s["W"])
    return a, b, msref.homography(a, b, levels=s["levels"], oriented=bool(s["oriented"]), max_hyp=s["max_hyp"], thr=s["thr"], min_inliers=s["min_inliers"], seed=s["seed"])


@functools.lru_cache(maxsize=None)
def _df_want():
    s = _SCALARS["df"]
    H, W = s["H"], s["W"]
    items = [dfref.flow_pair(H, W, 1.5, seed) for seed in (3, 4)]
    a, b = np.stack([i[0] for i in items]), np.stack([i[1] for i in items])
    m1 = np.ones((2, 1, H, W), np.float32)
    m1[:, :, 12:20, 25:36] = 0
    m2 = np.ascontiguousarray(np.broadcast_to(np.stack([i[2] for i in items]), (2, 3, H, W))).copy()
    m2[:, 1:] = 0                                                                    # only channel 0 counts
    res = [dfref.dense_flow(a[k], b[k], m1[k], m2[k], levels=s["levels"], iters=s["iters"], radius=s["radius"], damping=s["damping"]) for k in range(2)]
    return a, b, m1, m2, res


def _u16(x):
    return np.ascontiguousarray(x).astype(np.uint16)


def fixture(entry):
    """(contents {input operand: array}, expected {output operand: array}) of the entry's base record; an entry whose results lie in its
    workspace, or need a driver (seam_gc), has its own check in the GPU file and gives expected = None"""
    fam = family(entry)
    if fam == "ft":
        a, b, w = _ft_want()
        ins = dict(img=a, img1=a, img2=b, box=_u16(w["box1"]), kp=w["kp1"], kp1=w["kp1"], kp2=w["kp2"], desc1=w["desc1"], desc2=w["desc2"], matches=w["matches"],
                   count=w["count"].astype(np.int32))
        outs = dict(kp_out=w["kp1"], box_out=_u16(w["box1"]), desc_out=w["desc1"], nn_out=w["nn"], matches_out=w["matches"], count_out=w["count"].astype(np.int32),
                    motion_out=w["motion"], H_out=w["H"], info_out=w["info"], mask_out=w["mask"])
    elif fam == "ms":
        a, b, w = _ms_want()
        ins = dict(img=a, img1=a, img2=b, pyr=msref.pack_levels(w["pyr1"]).astype(np.uint8), box=_u16(msref.pack_levels(w["box1"])), kp=w["kp1"], bins=w["bins1"],
                   kp1=w["kp1"], kp2=w["kp2"], desc1=w["desc1"], desc2=w["desc2"], matches=w["matches"], count=w["count"].astype(np.int32))
        outs = dict(pyr_out=msref.pack_levels(w["pyr1"]).astype(np.uint8), kp_out=w["kp1"], bins_out=w["bins1"], box_out=_u16(msref.pack_levels(w["box1"])), desc_out=w["desc1"],
                    nn_out=w["nn"], matches_out=w["matches"], count_out=w["count"].astype(np.int32), motion_out=w["motion"], H_out=w["H"], info_out=w["info"],
                    mask_out=w["mask"], xy_out=w["xy"])
    elif fam == "df":
        a, b, m1, m2, res = _df_want()
        s = _SCALARS["df"]
        f = [r[2] for r in res]
        U = np.stack([r[2]["u"][0] for r in res])
        it = [dfref.iterate(f[k]["v1"][0], f[k]["v2"][0], f[k]["m1"][0], f[k]["m2"][0], U[k], s["radius"], s["damping"]) for k in range(2)]
        ins = dict(img1=a, img2=b, mask1=m1, mask2=m2, v1=np.stack([x["v1"][0] for x in f]).astype(np.int16), v2=np.stack([x["v2"][0] for x in f]).astype(np.int16),
                   m1=np.stack([x["m1"][0] for x in f]).astype(np.uint8), m2=np.stack([x["m2"][0] for x in f]).astype(np.uint8), u=U.astype(np.int32))
        outs = (dict(u_out=np.stack([x[0] for x in it]).astype(np.int32), support_out=np.stack([x[1] for x in it]).astype(np.uint8)) if entry == "st_dense_flow_iterate" else
                dict(flow_out=np.stack([r[0] for r in res]), support_out=np.stack([r[1] for r in res]).astype(np.uint8)))
        if entry == "st_dense_flow_pyramid":
            outs = None
    elif fam == "gc":
        s = _SCALARS["gc"]
        i1, i2 = gcref.smooth_texture_pair(s["H"], s["W"], 5)
        k1, k2 = gcref.bands(s["H"], s["W"])
        ins, outs = dict(img1=i1, img2=i2, mask1=k1, mask2=k2), None
    elif fam == "cr":
        s = _SCALARS["cr"]
        ys, xs = np.mgrid[0:s["H"], 0:s["W"]]
        k1 = ((xs < 25) & (ys > 1) & ~((ys == 9) & (xs == 7)))[None].astype(np.float32)
        k2 = ((xs > 12) & (ys < 17))[None].astype(np.float32)
        u = crref.union(k1, k2)
        ins, outs = dict(mask1=k1, mask2=k2), dict(info_out=np.array(crref.rect(u), np.int32), runs_out=crref.runs(u))
    else:
        s = _SCALARS["pm"]
        img, mask = pmref.scene("ramp", s["H"], s["W"]), pmref.masks(s["H"], s["W"])["corner"].astype(np.uint8)
        out, info, nnf, sad = pmref.patchmatch(img, mask, levels=s["levels"], iters=s["iters"], seed=s["seed"])
        ins, outs = dict(img=img, mask=mask), dict(out=out, info_out=np.array(info, np.int32), nnf_out=nnf, sad_out=sad)
    names = {x.name: x.role for x in entries()[entry]}
    return ({k: np.ascontiguousarray(v) for k, v in ins.items() if names.get(k) == "in"},
            None if outs is None else {k: np.ascontiguousarray(v) for k, v in outs.items() if names.get(k) == "out"})


def launching():
    return sorted(e for e in entries() if e not in HOST_ONLY)


# ---- part C: scenes of the corner cases ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def strip_pair(H, W):
    """img1, img2 fp32 [1,3,H,W] for a 64-wide strip: a shift of 24 px along the long side (chosen so that the restatement finds a valid model)"""
    motion = (24, 0, 0, 0, 0) if W > H else (0, 24, 0, 0, 0)
    return ftref.pair(H, W, motion, seed=4, sigma=1.0)[:2]


@functools.lru_cache(maxsize=None)
def batch_items(H, W):
    """four distinct pairs [1,3,H,W]"""
    return [ftref.pair(H, W, (3 + k, -2, 0.5 * k, 0, 0), seed=5 + k)[:2] for k in range(4)]


@functools.lru_cache(maxsize=None)
def flow_items(key):
    """img1, img2 fp32 [B,3,H,W]: one item per strip size; four distinct 16 x 16 items for key "batch" """
    if key == "batch":
        items = [dfref.flow_pair(16, 16, 1.0, seed, masked=False) for seed in (3, 4, 5, 6)]
    else:
        items = [dfref.flow_pair(key[0], key[1], 2.0, 3, masked=False)]
    return np.stack([i[0] for i in items]), np.stack([i[1] for i in items])


def thin_seam_scene(H, W):
    """img1, img2 [3,H,W], mask1, mask2 [1,H,W]: two bands along the long side that overlap over 150 px (five 32-wide tiles), textured"""
    long = max(H, W)
    t = np.arange(long)
    k1, k2 = (t < 2100), (t >= 1950)
    rng = np.random.default_rng(8)
    base = np.floor(100 + 60 * np.sin(t / 23.0))[None, None, :] + np.zeros((3, min(H, W), 1))
    i1, i2 = base.astype(np.float32), (base + rng.integers(0, 40, base.shape)).astype(np.float32)
    k1, k2 = (np.broadcast_to(k, (1, min(H, W), long)).astype(np.float32) for k in (k1, k2))
    if H > W:
        i1, i2, k1, k2 = (np.ascontiguousarray(v.transpose(0, 2, 1)) for v in (i1, i2, k1, k2))
    return tuple(np.ascontiguousarray(v) for v in (i1, i2, k1, k2))
