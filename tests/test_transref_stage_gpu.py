"""Per-stage gate of the TransRef network against fp64: every host stage of stitch_amd.transref.TransRefNet -- block (Block, Block_Ref,
Block_dec), nonlocal_block, refpa, patch_embed, convT, resblock, the clean convolution + tanh -- on its own, at small shapes the whole-network
golden never visits (H x W no multiple of sr, ragged key counts, odd sizes, H = 1), fed the stored input of
tests/golden/transref_stages*.npz (tools/make_transref_stage_golden.py: the reference's own submodule on the CPU, seeded weights 2024).

Bound: the control rule of tests/test_stage_fp64_gpu.py with the reference's recorded fp32 run as the control,
    e_rms(HIP) <= 2 max(e_rms(fp32), 2^-24),   e_max(HIP) <= 4 max(e_max(fp32), 2^-24),
e_rms(X) = |X - Y64|_2 / |Y64|_2, e_max(X) = max|X - Y64| / max|Y64|.  None is derived from a HIP measurement; every figure is recorded."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _transref_bounds as tb  # noqa: E402
from _measure import check  # noqa: E402

FLOOR = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return {f: np.load(os.path.join(GOLDEN, f)) for f in tb.STAGE_FILES}


@pytest.fixture(scope="module")
def net():
    from stitch_amd import transref as tr
    assert torch.cuda.is_available()
    return tr.Inpainter(seed=tb.STAGE_SEED, device="cuda", graph=False)._net()


def run_stage(net, name, ins):
    """the TransRefNet method of stage `name` on channels-last device inputs -> channels-last output"""
    kind, _, key, (H, W), _, args = tb.STAGES[name]
    if kind == "block":
        return net.block(ins[0], key, H, W, *args)
    if kind == "block_ref":
        return net.block(ins[0], key, H, W, *args, ref=ins[1])
    if kind == "nonlocal":
        return net.nonlocal_block(ins[0], key, H, W, ins[1])
    if kind == "refpa":
        return net.refpa(ins[0], ins[1], key, H, W)
    if kind == "embed":
        return net.patch_embed(ins[0], key, H, W, *args)[0]
    if kind == "convT":
        return net.convT(ins[0], key, H, W, act=args[0], res=ins[1] if len(ins) > 1 else None)
    if kind == "res":
        return net.resblock(ins[0], key, H, W, ins[1] if len(ins) > 1 else None)
    if kind == "clean":
        return net.conv(ins[0], key, H, W, 3, 1, 1, act="tanh")[0]
    raise KeyError(kind)


@pytest.mark.parametrize("name", list(tb.STAGES))
def test_stage_vs_fp64(gold, net, name):
    ins, ref, (c_rms, c_max) = tb.load_stage(gold, name)
    keep = [t.clone() for t in ins]
    dev = [t.cuda().contiguous() for t in ins]
    out = run_stage(net, name, dev)
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(ref.shape) == tb.stage_out_shape(name)
    assert all(torch.equal(d.cpu(), k) for d, k in zip(dev, keep)), "a stage wrote into its input"
    h_rms, h_max = tb.stage_errs(out.cpu(), ref)
    note = f"the reference's own fp32 run on the same input: e_rms {c_rms:.3e}, e_max {c_max:.3e}"
    failed = []
    for nm, val, bound in ((f"tr_stage_{name}_rms_over_ctl", h_rms / max(c_rms, FLOOR), 2.0), (f"tr_stage_{name}_max_over_ctl", h_max / max(c_max, FLOOR), 4.0)):
        try:
            check(nm, val, bound, inclusive=True, note=note)
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)
