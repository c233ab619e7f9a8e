"""The warm start without a GPU: the CPU restatement of the splat (tests/_forward_interp_ref.py) against the reference's own
scipy outputs (tests/golden/warmstart.npz, written by tools/make_warmstart_golden.py), its two stated deviations (ties, no valid
source), the C-ABI declaration and host-side argument checks, and an ISA guard on the built kernel."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import _forward_interp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "seamless-through-breaking-rethinking-image-stitching-for-optimal-alignment_amd")
LLVM = "/opt/rocm/llvm/bin"
MIN_GAP = 1e-9


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "warmstart.npz"))


def tie_field(gold):
    seed, H, W = (int(v) for v in gold["a_tie_seed_hw"])
    return np.random.default_rng(seed).integers(-3, 4, (2, H, W)).astype(np.float32)


def test_golden_has_the_fields_the_issue_asks_for(gold):
    names = list(gold["a_names"])
    shapes = {tuple(gold[f"a_{n}_in"].shape[1:]) for n in names}
    assert len(names) >= 6 and shapes == {(64, 64), (40, 72), (12, 16)}
    amps = [float(np.abs(gold[f"a_{n}_in"]).max()) for n in names]
    assert min(amps) < 1.0 and max(amps) > 30.0
    assert min(float(gold[f"a_{n}_valid_frac"]) for n in names) < 0.4
    assert bool(gold["b_seeded_zero_init_equals_cold"]) and bool(gold["b_damped_zero_init_equals_cold"])


def test_restatement_equals_the_reference_splat_bit_for_bit(gold):
    for n in gold["a_names"]:
        got = R.forward_interpolate(gold[f"a_{n}_in"])
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), gold[f"a_{n}_out"].view(np.int32)), n


def test_no_golden_field_has_a_tie(gold):
    """every query of every golden splat input: best and second-best fp64 squared distance more than 1e-9 apart, 0 queries excluded
    (so scipy's KD-tree order never decides a golden pixel)"""
    fields = [gold[f"a_{n}_in"] for n in gold["a_names"]] + [gold["c_f0_flow_lowres"][0], gold["c_f0_flow_lowres"][1]]
    for f in fields:
        _, gap = R.nearest_source(f, want_gap=True)
        assert gap.shape == (f.shape[1] * f.shape[2],) and gap.min() > MIN_GAP, gap.min()
    assert float(gold["b_seeded_fi_min_gap"]) > MIN_GAP and float(gold["b_damped_fi_min_gap"]) > MIN_GAP


def test_sequence_golden_init_is_the_splat_of_the_previous_frame(gold):
    assert not gold["c_f0_init"].any()
    assert np.array_equal(R.forward_interpolate(gold["c_f0_flow_lowres"]), gold["c_f1_init"])


def test_integer_field_ties_go_to_the_lowest_source_index(gold):
    f = tie_field(gold)
    idx, gap = R.nearest_source(f, want_gap=True)
    assert int((gap == 0).sum()) == int(gold["a_tie_queries_with_ties"]) > 1000
    px, py, valid = R.landing(f)
    H, W = f.shape[1:]
    for q in np.flatnonzero(gap == 0)[::37]:
        d = (q % W - px) ** 2 + (q // W - py) ** 2
        d[~valid] = np.inf
        assert idx[q] == np.flatnonzero(d == d.min())[0]
    # the generator recorded that scipy's own choice differs on such a field: the rule is a stated deviation, not scipy's behaviour
    assert int(gold["a_tie_px_differ_from_scipy"]) > 0


def test_all_invalid_gives_zeros_and_nan_sources_are_skipped():
    f = np.full((2, 12, 16), 100.0, np.float32)
    assert not R.forward_interpolate(f).any()
    f = R.generic_field(12, 16, 1.5, 3)
    g = f.copy()
    g[0, 4, 5] = np.nan
    g[1, 7, 2] = np.nan
    g[:, 0, 0] = np.inf
    _, _, valid = R.landing(g)
    assert not valid[4 * 16 + 5] and not valid[7 * 16 + 2] and not valid[0]
    out = R.forward_interpolate(g)
    assert np.isfinite(out).all()
    idx = R.nearest_source(g)
    assert not np.isin(idx, [0, 4 * 16 + 5, 7 * 16 + 2]).any()
    # where the skipped sources were not the winners before, nothing changes
    keep = ~np.isin(R.nearest_source(f), [0, 4 * 16 + 5, 7 * 16 + 2])
    assert np.array_equal(out.reshape(2, -1)[:, keep], R.forward_interpolate(f).reshape(2, -1)[:, keep])
    b = R.forward_interpolate(np.stack([f, g]))
    assert np.array_equal(b[0], R.forward_interpolate(f)) and np.array_equal(b[1], out)


def test_header_declares_the_new_symbols_and_the_host_rejects_bad_arguments():
    from stitch_amd._lib import declared_functions, lib
    decl = declared_functions()
    assert decl["st_flow_forward_interpolate"] == [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    assert decl["st_coords_grid_init"] == [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    dp, dq = C.c_void_p(256), C.c_void_p(1 << 20)       # never dereferenced: every call below is rejected on the host
    assert lib.st_flow_forward_interpolate(None, 0, dq, 1, 8, 8, None) == 1001
    assert lib.st_flow_forward_interpolate(dp, 0, None, 1, 8, 8, None) == 1001
    assert lib.st_flow_forward_interpolate(dp, 0, dp, 1, 8, 8, None) == 1001            # in place
    assert lib.st_flow_forward_interpolate(dp, 1, dq, 0, 8, 8, None) == 1001
    assert lib.st_flow_forward_interpolate(dp, 0, dq, 1, 0, 8, None) == 1001
    assert lib.st_flow_forward_interpolate(dp, 0, dq, 1, 256, 257, None) == 1001        # N > 65536
    assert lib.st_flow_forward_interpolate(dp, 0, dq, 65536, 8, 8, None) == 1001
    assert lib.st_coords_grid_init(dp, None, 1, 8, 8, None) == 1001
    assert lib.st_coords_grid_init(None, dp, 1, 8, 8, None) == 1001


def test_flowformer_forward_no_longer_refuses_flow_init():
    import inspect
    import stitch_amd
    from stitch_amd.flowformer import FlowFormer
    assert "NotImplementedError" not in inspect.getsource(FlowFormer.forward)
    for fn in (FlowFormer.flow_rows, FlowFormer.flow_rows_pair, FlowFormer._decoder, stitch_amd.FlowHomoAdpater.predict_flow,
               stitch_amd.FlowHomoAdpater.predict_flow_pair):
        assert inspect.signature(fn).parameters["flow_init"].default is None
    with pytest.raises(NotImplementedError):
        stitch_amd.SequenceStitcher(None, type="train")
    with pytest.raises(NotImplementedError):
        stitch_amd.SequenceStitcher(None, type="test_out", graphed=True)


def _code_object(tmp_path, marker):
    lib = os.path.join(PKG, "libstitch_gfx950.so")
    fb = str(tmp_path / "fatbin")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fb}", lib, str(tmp_path / "lib_copy.so")])
    data = open(fb, "rb").read()
    for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data):
        s = m.start()
        (n,) = struct.unpack_from("<Q", data, s + 24)
        p = s + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            co = data[s + off:s + off + size]
            if triple.endswith("gfx950") and marker in co:
                path = tmp_path / "flow_splat.co"
                path.write_bytes(co)
                return str(path)
    raise AssertionError("no gfx950 code object with the splat kernel in the library")


@pytest.mark.skipif(not os.path.exists(f"{LLVM}/llvm-objdump"), reason="needs the ROCm LLVM tools")
def test_splat_kernel_isa_no_packed_fp32_no_scratch(tmp_path):
    """the shipped library's code object (the build's own flags): both layouts of the kernel, no scratch, no spills, none of the
    packed fp32 instructions the build bans, and no fused fp64 multiply-add (the distance is two products and a sum)"""
    co = _code_object(tmp_path, b"flow_forward_interpolate_kernel")
    asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", co], capture_output=True, text=True, check=True).stdout
    bodies = dict((m.group(1), m.group(2)) for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", asm, re.S | re.M))
    names = [k for k in bodies if "flow_forward_interpolate_kernel" in k]
    assert len(names) == 2, sorted(bodies)
    for k in names:
        assert not re.search(r"v_pk_(mul|add|fma)_f32", bodies[k]), k
        assert "scratch_" not in bodies[k], k
        assert "v_fma_f64" not in bodies[k] and "v_mul_f64" in bodies[k] and "v_add_f64" in bodies[k], k
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    seen = 0
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", notes, re.S):
        if "flow_forward_interpolate_kernel" not in m.group(1):
            continue
        seen += 1
        body = m.group(2)
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", body), m.group(1)
        spill = re.search(r"\.vgpr_spill_count:\s+(\d+)", body)
        assert spill is None or int(spill.group(1)) == 0, m.group(1)
    assert seen == 2
