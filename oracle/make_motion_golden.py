"""Corner offsets of the CPU oracle's homography network for the end-to-end GPU tests (test infrastructure, CPU only).

    python -m oracle.make_motion_golden

Writes tests/golden/oracle_motion_512.npz.  The oracle's `homo_offsets` (ResNet-50 stages -> CCL -> regressor, torch-CPU fp32)
is not bit-stable across hosts: its result moves by ~1e-5 px with the CPU thread count and the instruction set the BLAS
kernels dispatch to.  With the seeded (chaotic) flow weights that difference becomes ~0.05 px of flow and hundreds of occlusion
pixels downstream, so a test that runs the oracle end to end from its own offsets compares against a different draw on every
host.  The tests start the oracle from these stored offsets instead (and check that the live network still reproduces them to
host tolerance); everything after the homography stage is evaluated live.  Generated with one CPU thread.
  quality_seeds / quality_shifts / quality_motion   tests/test_parity_gpu.py::test_quality_psnr_ssim_vs_oracle, 8 pairs
  chain_seed / chain_shift / chain_motion           tests/test_chain512_gpu.py `chain` fixture (type='test_out' on 512 x 512)
"""
from __future__ import annotations

import os

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "oracle_motion_512.npz")

QUALITY_SEEDS = [300 + i for i in range(8)]
QUALITY_SHIFTS = [(3 * (i % 5) - 6, 7 - 2 * (i % 7)) for i in range(8)]
CHAIN_SEED, CHAIN_SHIFT = 61, (5, -7)


def main():
    from oracle import geom, inputs, spec
    from oracle.nets import W, homo_offsets
    torch.set_num_threads(1)
    hw = W(spec.seeded_state_dict(1234), "homo_backbone.")
    with torch.no_grad():
        quality = [homo_offsets(hw, *inputs.structured_pair(512, 512, seed=s, shift=sh)) for s, sh in zip(QUALITY_SEEDS, QUALITY_SHIFTS)]
        a, b = inputs.structured_pair(512, 512, seed=CHAIN_SEED, shift=CHAIN_SHIFT)
        chain = homo_offsets(hw, geom.resize512(a), geom.resize512(b))
    np.savez_compressed(OUT, quality_seeds=np.array(QUALITY_SEEDS), quality_shifts=np.array(QUALITY_SHIFTS),
                        quality_motion=torch.cat(quality).numpy(), chain_seed=np.array(CHAIN_SEED), chain_shift=np.array(CHAIN_SHIFT),
                        chain_motion=chain.numpy())
    print(os.path.normpath(OUT))


if __name__ == "__main__":
    main()
