"""Golden vectors of the warm start (flow_init + forward_interpolate) from the REFERENCE's own code (CPU only; writes
tests/golden/warmstart.npz).

    python tools/make_warmstart_golden.py [--parts abc]

The reference is built by oracle.ref_harness.stubs.build_reference and its splat is core.utils.utils.forward_interpolate (imported,
not edited).  ``--parts`` regenerates only the named parts and keeps the others' keys of an existing file ((d) belongs to part c).

(a) splat     float fields (64x64, 40x72, 12x16; sub-pixel to 40 px; one with < 40 % valid points) and scipy's outputs, bit for
              bit.  Asserted here: the restatement (tests/_forward_interp_ref.py) equals scipy on every field, and for every query of
              every field the best and second-best fp64 squared distances differ by more than 1e-9 (no ties, 0 queries excluded).
              Also recorded: scipy against the lowest-index rule on an integer field (ties: scipy's order is its KD-tree's).
(b) network   flow_backbone(a, b, {}, flow_init=fi), fi = the splat of the previous structured pair's flow_lowres: damped weights at
              512x512, seeded weights at 96x128; 8 vs 1 thread spread as *_floor_*; zero init == cold call; seeded: the fp64 run.
(c) sequence  three frames of a slowly moving structured pair through test_eval (damped weights, 512x512), each direction's flow
              call given flow_init = forward_interpolate(previous flow_lowres); the chain rerun with 1 thread as the floor.
(d) control   frames 2 and 3 again, the init taken from the previous low-res flow perturbed by uniform noise of 2.5e-4 / 8 low-res px
              (the GPU-vs-reference flow gap measured on these weights, damped_e2e_flow_max_px): the reference's own movement.
"""
from __future__ import annotations

import copy
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _forward_interp_ref as R  # noqa: E402
from oracle import inputs, spec  # noqa: E402
from oracle.ref_harness import stubs  # noqa: E402
from oracle.ref_harness.make_goldens import OUT, checksum, packbits, sub  # noqa: E402

SHIPPED = dict(test_not_use_combine_h_flow=True, use_forward=False, use_fb_consistency_mask=True, use_whole_resolution=False)
PATH = os.path.join(OUT, "warmstart.npz")
MIN_GAP = 1e-9
SPLAT_FIELDS = (("f64a", 64, 64, 0.4, 1), ("f64b", 64, 64, 25.0, 3), ("f40a", 40, 72, 3.0, 4), ("f40b", 40, 72, 40.0, 5),
                ("f12a", 12, 16, 1.5, 7), ("f12b", 12, 16, 12.0, 6))
SEQ_SHIFTS = ((5, -9), (6, -10), (7, -11))
PERTURB = 2.5e-4 / 8


def _ref_splat():
    stubs.install()
    from core.utils.utils import forward_interpolate
    return forward_interpolate


def _mx(x, y):
    return np.array(float((x - y).abs().max()))


def _splat_checked(fi, low, what):
    """the reference's splat of one [2,H,W] field, with the no-tie condition and the restatement asserted on it"""
    out = fi(low).numpy()
    idx, gap = R.nearest_source(low.numpy(), want_gap=True)
    assert gap.min() > MIN_GAP, (what, gap.min())
    assert np.array_equal(out, R.forward_interpolate(low.numpy())), what
    return torch.from_numpy(out)[None], float(gap.min())


def part_a(rec):
    fi = _ref_splat()
    names = []
    for name, H, W, amp, seed in SPLAT_FIELDS:
        f = R.generic_field(H, W, amp, seed)
        _, _, valid = R.landing(f)
        out, gap = _splat_checked(fi, torch.from_numpy(f), name)
        rec[f"a_{name}_in"], rec[f"a_{name}_out"] = f, out[0].numpy()
        rec[f"a_{name}_min_gap"], rec[f"a_{name}_valid_frac"] = np.array(gap), np.array(valid.mean())
        names.append(name)
        print(f"(a) {name} {H}x{W} amp {amp}: valid {valid.mean():.3f} min gap {gap:.3e}", flush=True)
    assert min(float(rec[f"a_{n}_valid_frac"]) for n in names) < 0.4
    rec["a_names"] = np.array(names)
    z = np.zeros((2, 12, 16), np.float32)
    assert np.array_equal(fi(torch.from_numpy(z)).numpy(), z)                   # the all-zero field: every query has its own source
    # an integer-valued field: exact ties, where scipy's choice is its KD-tree's and the lowest-index rule is a stated deviation
    rng = np.random.default_rng(9)
    ti = rng.integers(-3, 4, (2, 64, 64)).astype(np.float32)
    _, gap = R.nearest_source(ti, want_gap=True)
    rec["a_tie_seed_hw"] = np.array([9, 64, 64])                 # rng.integers(-3, 4, (2, H, W)) of default_rng(seed): not stored
    rec["a_tie_queries_with_ties"] = np.array(int((gap == 0).sum()))
    rec["a_tie_px_differ_from_scipy"] = np.array(int((fi(torch.from_numpy(ti)).numpy() != R.forward_interpolate(ti)).any(0).sum()))
    print("(a) integer field: queries with ties", rec["a_tie_queries_with_ties"], "pixels != scipy", rec["a_tie_px_differ_from_scipy"], flush=True)


def _flow_case(rec, p, sd, h, w, fp64):
    fi = _ref_splat()
    model, _ = stubs.build_reference(sd, overlay=SHIPPED)
    fb = model.flow_backbone
    a0, b0 = inputs.structured_pair(h, w, seed=7) if h == 512 else inputs.structured_pair(h, w, seed=3, shift=(2, -3))
    a1, b1 = inputs.structured_pair(h, w, seed=7, shift=(6, -10)) if h == 512 else inputs.structured_pair(h, w, seed=3, shift=(3, -4))
    with torch.no_grad():
        torch.set_num_threads(8)
        t = time.time()
        _, low0 = fb(a0, b0, {})
        print(f"(b) {p} one forward: {time.time() - t:.1f} s", flush=True)
        init, gap = _splat_checked(fi, low0[0], p + "fi")
        up8, low8 = fb(a1, b1, {}, flow_init=init)
        upc, lowc = fb(a1, b1, {})
        upz, lowz = fb(a1, b1, {}, flow_init=torch.zeros_like(init))
        torch.set_num_threads(1)
        up1, low1 = fb(a1, b1, {}, flow_init=init)
        torch.set_num_threads(8)
        rec.update({p + "fi": init.numpy(), p + "fi_min_gap": np.array(gap), p + "flow_lowres": low8.numpy(), p + "flow_up_cs": checksum(up8),
                    p + "flow_up_sub": sub(up8, 4 if h == 512 else 1), p + "floor_flow_up_max_px": _mx(up8, up1),
                    p + "floor_flow_lowres_max": _mx(low8, low1), p + "zero_init_equals_cold": np.array(torch.equal(upz, upc) and torch.equal(lowz, lowc)),
                    p + "warm_vs_cold_flow_up_max_px": _mx(up8, upc), p + "flow_absmax": np.array(float(up8.abs().max()))})
        assert bool(rec[p + "zero_init_equals_cold"])
        if fp64:
            fb64 = copy.deepcopy(fb).double()
            up64, _ = fb64(a1.double(), b1.double(), {}, flow_init=init.double())
            rec[p + "flow_up_fp64_sub"] = sub(up64, 2)
            rec[p + "fp32_to_fp64_max_px"] = np.array(float((up8.double() - up64).abs().max()))
    print(f"(b) {p}", {k[len(p):]: v.tolist() for k, v in rec.items() if k.startswith(p) and v.size == 1}, flush=True)


def part_b(rec):
    _flow_case(rec, "b_seeded_", spec.seeded_state_dict(1234), 96, 128, fp64=True)
    _flow_case(rec, "b_damped_", spec.damped_state_dict(1234), 512, 512, fp64=False)


class _WarmFlow:
    """stands in for the reference model's predict_flow (flowHomoAdpater.py:63-70): the same call with flow_init; test_eval calls it
    for a->b first, then b->a"""

    def __init__(self, model):
        self.fb, self.init, self.low, self.n = model.flow_backbone, [None, None], [None, None], 0

    def __call__(self, x, y):
        d, self.n = self.n, self.n + 1
        up, low = self.fb(x, y, {}, flow_init=self.init[d])
        self.low[d] = low
        return [up]


def _frame(model, k, inits):
    a, b = inputs.structured_pair(512, 512, seed=7, shift=SEQ_SHIFTS[k])
    wf = _WarmFlow(model)
    wf.init = list(inits)
    model.predict_flow = wf
    try:
        with torch.no_grad():
            o = model(a, b, type="test_eval")
    finally:
        del model.predict_flow
    assert wf.n == 2
    return o, wf.low


def _chain(model, fi, rec=None, perturb=None):
    """three frames; returns per frame (outputs, inits used [2,2,H1,W1]).  perturb: a generator -- the inits of frames 2 and 3 come from the
    UNPERTURBED chain's previous low-res flow (rec: that chain's frames) plus uniform noise, and the chain itself is not advanced with them."""
    frames, inits = [], [None, None]
    for k in range(3):
        if perturb is not None:
            if k == 0:
                frames.append(None)
                continue
            prev = [rec[k - 1][2][d] for d in range(2)]
            inits = [fi(p + PERTURB * (2 * torch.rand(p.shape, generator=perturb) - 1)).unsqueeze(0) for p in prev]
        t = time.time()
        o, low = _frame(model, k, inits)
        used = torch.zeros(2, 2, 64, 64) if inits[0] is None else torch.cat(inits)
        frames.append((o, used, torch.cat(low)))
        print(f"    frame {k}: {time.time() - t:.1f} s", flush=True)
        if perturb is None:
            inits = [_splat_checked(fi, l[0], f"frame {k} dir {d}")[0] for d, l in enumerate(low)]
    return frames


def part_cd(rec):
    fi = _ref_splat()
    model, _ = stubs.build_reference(spec.damped_state_dict(1234), overlay=SHIPPED)
    torch.set_num_threads(8)
    f8 = _chain(model, fi)
    torch.set_num_threads(1)
    f1 = _chain(model, fi)
    torch.set_num_threads(8)
    rec["c_shifts"] = np.array(SEQ_SHIFTS)
    for k, ((o, init, low), (o1, _, _)) in enumerate(zip(f8, f1)):
        p = f"c_f{k}_"
        f = o["flow_predictions"][0]
        rec.update({p + "init": init.numpy(), p + "flow_lowres": low.numpy(), p + "H": o["H"].numpy(), p + "flow_sub": sub(f, 8),
                    p + "flow_cs": checksum(f), p + "final_sub": sub(o["final_warp_output"][:, 0:4], 8),
                    p + "output_H_sub": sub(o["output_H"][:, 0:4], 16), p + "occ_bits": packbits(o["origin_occlusion_mask"]),
                    p + "overlap_bits": packbits(o["overlap"]),
                    p + "floor_flow_max_px": _mx(f, o1["flow_predictions"][0]), p + "floor_H_max": _mx(o["H"], o1["H"]),
                    p + "floor_occ_flips": np.array(int((o["origin_occlusion_mask"] != o1["origin_occlusion_mask"]).sum())),
                    p + "floor_final_max": _mx(o["final_warp_output"], o1["final_warp_output"])})
        if k == 0:                                         # the cold frame: the existing end-to-end golden's case; flow only
            for key in ("final_sub", "output_H_sub"):
                del rec[p + key]
        else:                                              # (frame 1's init is the splat of frame 0's: kept once, for the CPU test)
            del rec[p + "flow_lowres"]
        print(f"(c) frame {k}", {key[len(p):]: v.tolist() for key, v in rec.items() if key.startswith(p + "floor")}, flush=True)
    # ---- (d): the same frames with the init from a perturbed previous low-res flow ------------------------------------------
    fd = _chain(model, fi, rec=f8, perturb=torch.Generator().manual_seed(5))
    rec["d_perturb_lowres_px"] = np.array(PERTURB)
    for k in (1, 2):
        o, init, _ = fd[k]
        f = o["flow_predictions"][0]
        rec[f"d_f{k}_flow_sub"] = sub(f, 8)
        rec[f"d_f{k}_init_moved_max"] = np.array(float((init - torch.from_numpy(rec[f"c_f{k}_init"])).abs().max()))
        d = np.abs(rec[f"d_f{k}_flow_sub"] - rec[f"c_f{k}_flow_sub"])
        rec[f"d_f{k}_flow_moved_max_px"], rec[f"d_f{k}_flow_moved_p99_px"] = np.array(d.max()), np.array(np.percentile(d, 99))
        rec[f"d_f{k}_occ_flips"] = np.array(int(np.unpackbits(packbits(o["origin_occlusion_mask"]) ^ rec[f"c_f{k}_occ_bits"]).sum()))
        print(f"(d) frame {k}: init moved {float(rec[f'd_f{k}_init_moved_max']):.3e} low-res px, flow moved max {d.max():.3e} p99 "
              f"{np.percentile(d, 99):.3e} px, occ flips {int(rec[f'd_f{k}_occ_flips'])}", flush=True)


def main():
    parts = "abc"
    if "--parts" in sys.argv:
        parts = sys.argv[sys.argv.index("--parts") + 1]
    torch.manual_seed(0)
    torch.set_num_threads(8)
    rec = dict(np.load(PATH)) if os.path.exists(PATH) and parts != "abc" else {}
    if "a" in parts:
        part_a(rec)
    if "b" in parts:
        part_b(rec)
    if "c" in parts:
        part_cd(rec)                                           # (d) perturbs (c)'s own low-res flows: one part
    np.savez_compressed(PATH, **rec)
    print(PATH, os.path.getsize(PATH))


if __name__ == "__main__":
    main()
