"""Stage fixtures of the TransRef network from the REFERENCE's own submodules (build container only; writes
tests/golden/transref_stages.npz and tests/golden/transref_stages_refpa.npz).

    python tools/make_transref_stage_golden.py            # writes the two files
    python tools/make_transref_stage_golden.py --check    # recomputes every stage and compares it with the committed files

Builds the reference's TransRef_Base twice (tools/make_transref_golden.build_reference: fp32 and fp64), loads
stitch_amd.transref.seeded_state_dict(2024) into both and runs every submodule of tests/_transref_bounds.STAGES on the CPU on that
table's seeded inputs: Block of the four encoder stages, Block_Ref, Block_dec, NONLocalBlock2D + extra, RefPA1..3, OverlapPatchEmbed
k7s4 / k3s2, both transposed convolutions, ResidualBlock with and without skip, clean + tanh.  Stored per stage: the fp32 input(s)
(channels-last), the fp64 output and the fp32 run's e_rms / e_max against it -- the control of tests/test_transref_stage_gpu.py.  The
fp32 output itself is not kept.  Data only; the layout of the two files is described in tests/_transref_bounds.py.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def nchw(x, H, W):
    return x.reshape(H, W, -1).permute(2, 0, 1)[None]


def cl(y):
    return y[0].permute(1, 2, 0).reshape(-1, y.shape[1])


def run_stage(net, name, ins):
    """the reference's submodule of stage `name` on channels-last inputs of the net's dtype -> channels-last output"""
    import _transref_bounds as tb
    kind, ref_key, _, (H, W), _, _ = tb.STAGES[name]
    m = net.get_submodule(ref_key)
    if kind == "block":
        return m(ins[0][None], H, W)[0]
    if kind == "block_ref":
        return m(ins[0][None], H, W, ins[1][None])[0]
    if kind == "nonlocal":
        return cl(m(nchw(ins[0], H, W)) + nchw(ins[1], H, W))
    if kind == "refpa":
        return cl(m(nchw(ins[0], H, W).contiguous(), nchw(ins[1], H, W).contiguous()))
    if kind == "embed":
        return m(nchw(ins[0], H, W))[0][0]
    if kind == "convT":
        y = m(nchw(ins[0], H, W))
        return cl(y + nchw(ins[1], 2 * H, 2 * W) if len(ins) > 1 else y)
    if kind == "res":
        y = m(nchw(ins[0], H, W))
        return cl(y + nchw(ins[1], H, W) if len(ins) > 1 else y)
    if kind == "clean":
        return cl(torch.tanh(m(nchw(ins[0], H, W))))
    raise KeyError(kind)


def reference_nets():
    import stitch_amd.transref as tr
    from make_transref_golden import build_reference
    import _transref_bounds as tb
    sd = tr.seeded_state_dict(tb.STAGE_SEED)
    nets = []
    for dt in (torch.float32, torch.float64):
        net = build_reference()
        net.load_state_dict(sd, strict=True)
        nets.append(net.to(dt).eval())
    return nets


def stage_record(nets, name):
    """-> (fp32 inputs, fp64 output as the fixture will give it back, (e_rms, e_max) of the fp32 run against that)"""
    import _transref_bounds as tb
    ins = tb.stage_inputs(name)
    with torch.no_grad():
        o32 = run_stage(nets[0], name, ins)
        o64 = run_stage(nets[1], name, [t.double() for t in ins])
    assert tuple(o64.shape) == tb.stage_out_shape(name), (name, o64.shape)
    if tb.STAGES[name][0] == "refpa":
        back = tb.unpack64(*tb.pack64(o64))
        ulp = np.spacing(np.abs(o64.float().numpy()))
        assert float(((back - o64).abs() / torch.from_numpy(ulp).double()).max()) <= 2.0 ** -8
        o64 = back
    return ins, o64.contiguous(), tb.stage_errs(o32, o64)


def main():
    import _transref_bounds as tb
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    nets = reference_nets()
    files = {f: {} for f in tb.STAGE_FILES}
    for name in tb.STAGES:
        ins, o64, e32 = stage_record(nets, name)
        z = files[tb.stage_file(name)]
        z[f"{name}.e32"] = np.array(e32, dtype=np.float64)
        if tb.STAGES[name][0] == "refpa":
            for j, t in enumerate(ins):
                z[f"{name}.in{j}"] = (t * 16).round().to(torch.int8).numpy()
            hi, lo = tb.pack64(o64)
            z[f"{name}.out_hi"], z[f"{name}.out_lo"] = hi.numpy(), lo.numpy()
        else:
            for j, t in enumerate(ins):
                z[f"{name}.in{j}"] = t.numpy()
            z[f"{name}.out64"] = o64.numpy()
        print(f"{name:14s} out {tuple(o64.shape)}  fp32 e_rms {e32[0]:.3e} e_max {e32[1]:.3e}")
    for f, z in files.items():
        path = os.path.join(GOLDEN, f)
        np.savez_compressed(path, **z)
        size = os.path.getsize(path)
        print(f"{f}: {len(z)} arrays, {size} bytes")
        assert size <= tb.STAGE_FILE_CAP, (f, size)


def check():
    """the committed fixture is what this tool computes: outputs to 1e-11 (RefPA: 2^-30, its int8 residual re-encoded) of the largest value,
    the fp32 controls to 5 % (rms) and 25 % (max)"""
    import _transref_bounds as tb
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    gold = {f: np.load(os.path.join(GOLDEN, f)) for f in tb.STAGE_FILES}
    nets = reference_nets()
    bad = []
    for name in tb.STAGES:
        ins, out, e32 = tb.load_stage(gold, name)
        new_ins, o64, e = stage_record(nets, name)
        tol = 2.0 ** -30 if tb.STAGES[name][0] == "refpa" else 1e-11
        if not all(torch.equal(a, b) for a, b in zip(ins, new_ins)) or float((o64 - out).abs().max()) > tol * float(out.abs().max()) or \
                abs(e[0] - e32[0]) > 0.05 * e32[0] or abs(e[1] - e32[1]) > 0.25 * e32[1]:
            bad.append(name)
    print("stages that differ from the fixture:", bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(check() if "--check" in sys.argv[1:] else main())
