"""UDIS-D evaluation harness (re-statement of the reference's evaluate.py:21-107).

One process per GPU: the test pairs are sharded round-robin (``dist.shard_indices``), each rank runs
``model(image1, image2, type="test_eval")`` and the masked PSNR / SSIM kernel on its pairs, one all-gather
collects the per-pair metrics, and every rank computes the reference's summary (descending sort, slices
[0:331], [331:663], [663:-1], means).  JPEG decoding uses PIL (the reference reads through PIL as well,
core/utils/frame_utils.py); cv2 is not needed on this path.

The default loop is a software pipeline (``EvalPipeline``): JPEG pairs are decoded ahead by a small thread pool (PIL releases
the GIL while it decodes), each of k pairs in flight owns a HIP stream, pinned staging buffers and ONE hipGraph that holds the
whole per-pair work -- uint8 HWC -> float CHW, ``forward(type="test_eval")``, the metric kernels -- and the per-pair (psnr, ssim)
rows stay in a device table until one copy at the end.  The host therefore does per pair: two decodes (off-thread), one memcpy
into pinned memory, two async H2D copies, one graph launch and one 16-byte device copy; it never waits for the GPU inside the
loop (the reference's loop synchronises four times per batch, evaluate.py:38-50).  ``pipelined=False`` keeps the plain
one-pair-at-a-time loop (eager launches, ``.cpu()`` per pair): same kernels, same bits -- ``tests/test_harness_gpu.py``.

``gpu_decode=True`` (default off) moves the JPEG decode onto the device: the worker threads only read and probe the files
(``ops.jpeg_probe``), the compressed bytes go through the slot's pinned buffer and the copy stream, and the two decodes
(``ops.jpeg_decode``, csrc/jpeg_dec.hip: Pillow's pixels bit for bit) run on the slot's stream straight into its uint8 staging
buffers, eagerly, before the graph replay -- their launch shapes depend on the file.  Their status words are read back with the
metric table; a nonzero one raises and names the file.  A work item with a file the decoder does not take (progressive, grey,
restart intervals, ..., or H * W not a multiple of 4) goes the Pillow path unchanged, with one printed line."""
from __future__ import annotations

import glob
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import dist as sdist
from . import ops


def _decode_rgb8(path):
    """core/datasets.py:381-384: PIL decode -> uint8 [H,W,3] (grey images tiled to 3 channels, alpha dropped)."""
    from PIL import Image
    arr = np.array(Image.open(path)).astype(np.uint8)
    if arr.ndim == 2:
        arr = np.tile(arr[..., None], (1, 1, 3))
    return np.ascontiguousarray(arr[..., :3])


class _JpegPair:
    """one pair as the worker thread leaves it with gpu_decode: the two files' bytes and their probes"""
    __slots__ = ("data", "info", "paths", "shape")

    def __init__(self, data, info, paths):
        self.data, self.info, self.paths = data, info, paths
        self.shape = (info[0].H, info[0].W, 3)


def _read_jpeg_pair(paths):
    """the files of a pair and their probes, or the reason why the pair keeps the Pillow path"""
    data, info = [], []
    for path in paths:
        with open(path, "rb") as f:
            d = f.read()
        i = ops.jpeg_probe(d, restart=True)
        if i is None:
            return None, f"{path} is outside the GPU decoder's contract"
        if i.ncomp != 3:
            return None, f"{path} is grey"
        if (i.H * i.W) % 4:
            return None, f"{path}: {i.H}x{i.W} is not a size of the uint8 path"
        data.append(d)
        info.append(i)
    if (info[0].H, info[0].W) != (info[1].H, info[1].W):
        return None, f"{paths[0]} and {paths[1]} differ in size"
    return _JpegPair(data, info, paths), None


class UDISDataset:
    """test branch of core/datasets.py:329-389: sorted input1/*.jpg, input2/*.jpg -> float RGB [3,H,W] in 0..255."""

    def __init__(self, data_dir, phase="testing"):
        assert phase == "testing", "only the evaluation split is on the stitching path"
        root = os.path.join(data_dir, phase)
        self.image_list = list(zip(sorted(glob.glob(os.path.join(root, "input1", "*.jpg"))),
                                   sorted(glob.glob(os.path.join(root, "input2", "*.jpg")))))

    def __len__(self):
        return len(self.image_list)

    def load_u8(self, index):
        """the pair as the decoder leaves it: two uint8 [H,W,3] arrays (the pipelined harness converts on the GPU)."""
        p1, p2 = self.image_list[index]
        return _decode_rgb8(p1), _decode_rgb8(p2)

    def __getitem__(self, index):
        a, b = self.load_u8(index)
        return (torch.from_numpy(a).permute(2, 0, 1).float(), torch.from_numpy(b).permute(2, 0, 1).float(),
                self.image_list[index])


def summarize(psnr_list, ssim_list):
    """evaluate.py:68-106 (sort descending; easy/mid/hard = [0:331], [331:663], [663:-1])."""
    p = sorted((float(x) for x in psnr_list), reverse=True)
    s = sorted((float(x) for x in ssim_list), reverse=True)
    pe, pm, ph = sdist.split_easy_mid_hard(p)
    se, sm, sh = sdist.split_easy_mid_hard(s)
    mean = lambda v: float(np.mean(v)) if len(v) else float("nan")
    return {"avg_psnr": mean(p), "avg_ssim": mean(s), "easy_psnr": mean(pe), "mid_psnr": mean(pm), "hard_psnr": mean(ph),
            "easy_ssim": mean(se), "mid_ssim": mean(sm), "hard_ssim": mean(sh)}


class _Slot:
    """One pair (or batch of same-shaped pairs) in flight: a HIP stream, pinned staging, a device staging buffer the copy stream
    fills, the static float inputs and the hipGraph of the per-pair work (forward + metric) for one input shape."""

    def __init__(self, model, device, shape, u8):
        self.stream = torch.cuda.Stream(device=device)
        self.h2d_done = torch.cuda.Event()              # copy stream: pinned -> stage finished (pinned buffers reusable)
        self.consumed = torch.cuda.Event()              # slot stream: stage -> static inputs finished (stage reusable)
        self.inflight = deque()                         # completion events of this slot's launches (host throttle)
        B, H, W = shape
        host_shape = (B, H, W, 3) if u8 else (B, 3, H, W)
        dt = torch.uint8 if u8 else torch.float32
        self.u8 = u8
        self.pin = [torch.empty(host_shape, dtype=dt).pin_memory() for _ in range(2)]
        self.pin_np = [p.numpy() for p in self.pin]
        self.stage = [torch.empty(host_shape, dtype=dt, device=device) for _ in range(2)]
        self.inputs = [torch.zeros((B, 3, H, W), dtype=torch.float32, device=device) for _ in range(2)]
        self.device = device
        self.jpin = self.jdev = self.jws = None         # gpu_decode: pinned / device bytes of the slot's files, decoder workspace
        self.jconsumed = torch.cuda.Event()             # slot stream: the decodes out of jdev finished (jdev reusable)
        self.metric = torch.empty((B, 2), dtype=torch.float64, device=device)
        ws = ops.new_workspace(device)                 # this graph's own split-K slabs (graphs replay concurrently)

        def body():
            out = model(self.inputs[0], self.inputs[1], type="test_eval")
            ops.masked_psnr_ssim(self.inputs[0], out["final_warp_output"], out=self.metric)        # evaluate.py:44-59

        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), ops.workspace_scope(ws):
            for _ in range(2):                          # warm-up: weight prepack, constant tables, LDS attributes
                body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), ops.workspace_scope(ws):
            body()
        self._keep = ws

    def jpeg_buffers(self, nbytes, ws_bytes):
        """the slot's byte buffers and decoder workspace, grown (rarely) when a work item needs more"""
        if self.jpin is None or self.jpin.numel() < nbytes or self.jws.numel() < ws_bytes:
            self.stream.synchronize()                   # nothing of this slot reads the old buffers any more
            self.h2d_done.synchronize()
            cap = max(2 * nbytes, 1 << 20, 0 if self.jpin is None else self.jpin.numel())
            self.jpin = torch.empty((cap,), dtype=torch.uint8).pin_memory()
            self.jdev = torch.empty((cap,), dtype=torch.uint8, device=self.device)
            self.jws = torch.empty((max(2 * ws_bytes, 0 if self.jws is None else self.jws.numel()),), dtype=torch.uint8, device=self.device)
        return self.jpin, self.jdev, self.jws

    def unstage(self):
        """device staging -> the graph's static float inputs, on the slot's stream (core/datasets.py:383-386 on the GPU)."""
        for st, dst in zip(self.stage, self.inputs):
            if self.u8:
                ops.load_rgb8(st, out=dst)
            else:
                dst.copy_(st, non_blocking=True)


class EvalPipeline:
    """k pairs in flight, decode-ahead, metric on the device until the end (module docstring).  Kept on the model
    (``model._eval_pipeline``) so that the graphs are captured once per (input shape, slot).

    Per pair the host (1) takes the decoded arrays from the worker pool, (2) copies them into the slot's pinned buffers, (3)
    enqueues the two H2D copies on a COPY stream of its own -- an H2D copy enqueued on the slot's compute stream would sit behind
    the slot's previous graph and the next graph behind the copy: measured 75.6 instead of 81.8 pairs/s
    (a phase-timed copy of this loop, round 4; tools/harness_profile.py sweeps streams / decode threads) -- and (4) on the slot's stream: wait for the copy, uint8 HWC -> float CHW into the graph's static
    inputs, replay the graph, copy the (psnr, ssim) row into the device table.  At most two launches per slot are outstanding
    (the host waits on the completion event of the launch before the previous one), so the GPU always has work queued and the
    host never runs more than 2 k pairs ahead."""

    MAX_OUTSTANDING = 2
    MAX_SHAPES = 4          # distinct (batch, H, W, dtype) kept captured; each costs nslots x (a forward's activations + 64 MiB workspace + pinned staging)

    def __init__(self, model, device, streams=3, decode_workers=None, gpu_decode=False):
        self.model, self.device, self.nslots = model, device, max(1, int(streams))
        self.gpu_decode = bool(gpu_decode)
        try:
            ncpu = len(os.sched_getaffinity(0))
        except AttributeError:
            ncpu = os.cpu_count() or 1
        self.workers = decode_workers or max(2, min(4, ncpu // 2))     # 1.7 ms per 512x512 pair and thread: 4 threads feed ~2 000 pairs/s
        self.copy_stream = torch.cuda.Stream(device=device)
        self._slots = {}                # (shape, u8, branch) -> {slot index: _Slot}, in least-recently-used order
        self._gen = None

    def _slot(self, k, shape, u8):
        """The slot (stream + graph) number k for this input shape; captured on first use.  The cache is bounded: a dataset of many image
        sizes (or ragged batch tails) evicts the least recently used SHAPE -- its graphs, private pools and pinned buffers go with it.
        The model's test_eval branch and its (homo_source, flow_source) are part of the key: a cfg flag flipped after a capture (only_homo, use_combine_h_flow) captures anew
        instead of replaying the other branch's graph."""
        branch = self.model.eval_branch() if hasattr(self.model, "eval_branch") else None
        sources = self.model.sources() if hasattr(self.model, "sources") else None
        key = (shape, u8, branch, sources)
        group = self._slots.pop(key, None)
        if group is None:
            group = {}
            while len(self._slots) >= self.MAX_SHAPES:
                old = self._slots.pop(next(iter(self._slots)))
                for sl in old.values():
                    sl.stream.synchronize()
                    sl.graph = None
                old.clear()
        self._slots[key] = group                        # most recently used last
        if k not in group:
            group[k] = _Slot(self.model, self.device, shape, u8)
        return group[k]

    def n_captured(self):
        return sum(len(g) for g in self._slots.values())

    def _check_weights(self):
        """Graphs replay against the packed weights they were captured with: drop them all when the model's weights changed identity since
        (sub-module ``load_state_dict``, ``.to()`` / ``.float()``, in-place parameter writes) -- ``FlowHomoAdpater.weights_generation``."""
        gen = self.model.weights_generation(deep=True) if hasattr(self.model, "weights_generation") else None
        if gen != self._gen:
            if self._slots:
                torch.cuda.synchronize(self.device)
            self._slots.clear()
            self._gen = gen

    def _load(self, dataset, idx):
        """host side of one work item: decode (worker thread) -> list of (array pair) + whether they are uint8 HWC.  With gpu_decode a
        JPEG dataset's work item is a list of `_JpegPair` (bytes and probes) instead, unless one of its files keeps the Pillow path."""
        if self.gpu_decode and hasattr(dataset, "image_list") and hasattr(dataset, "load_u8"):
            pairs = []
            for i in idx:
                pair, why = _read_jpeg_pair(dataset.image_list[i])
                if pair is None:
                    print(f"gpu_decode: pairs {list(idx)} decoded with Pillow ({why})", flush=True)
                    break
                pairs.append(pair)
            else:
                return pairs, True
        if hasattr(dataset, "load_u8"):
            return [dataset.load_u8(i) for i in idx], True
        items = [dataset[i] for i in idx]              # generic dataset: float [3,H,W] tensors, uploaded as they are
        return [(it[0].float().contiguous().numpy(), it[1].float().contiguous().numpy()) for it in items], False

    def _launch(self, slot, sub, table, row):
        while len(slot.inflight) >= self.MAX_OUTSTANDING:
            slot.inflight.popleft().synchronize()
        slot.h2d_done.synchronize()                    # the previous H2D out of this slot's pinned buffers (long done)
        for i, (a, b) in enumerate(sub):
            np.copyto(slot.pin_np[0][i], a)
            np.copyto(slot.pin_np[1][i], b)
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(slot.consumed)         # the stage buffers' previous content has been converted
            slot.stage[0].copy_(slot.pin[0], non_blocking=True)
            slot.stage[1].copy_(slot.pin[1], non_blocking=True)
            slot.h2d_done.record()
        with torch.cuda.stream(slot.stream):
            slot.stream.wait_event(slot.h2d_done)
            slot.unstage()
            slot.consumed.record()
            slot.graph.replay()
            table[row:row + len(sub)].copy_(slot.metric, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            slot.inflight.append(done)

    def _launch_jpeg(self, slot, sub, table, row, status, srow):
        """`_launch` with the decode on the device: bytes -> pinned -> device on the copy stream, two decodes per pair on the slot's stream"""
        while len(slot.inflight) >= self.MAX_OUTSTANDING:
            slot.inflight.popleft().synchronize()
        offs, total = [], 0
        for p in sub:
            for d in p.data:
                offs.append(total)
                total += (len(d) + 15) & ~15
        ws_bytes = max(ops.jpeg_dec_workspace_bytes(i) for p in sub for i in p.info)
        jpin, jdev, jws = slot.jpeg_buffers(total, ws_bytes)
        slot.h2d_done.synchronize()                    # the previous H2D out of this slot's pinned buffers (long done)
        jnp = jpin.numpy()
        k = 0
        for p in sub:
            for d in p.data:
                jnp[offs[k]:offs[k] + len(d)] = np.frombuffer(d, np.uint8)
                k += 1
        with torch.cuda.stream(self.copy_stream):
            self.copy_stream.wait_event(slot.jconsumed)        # the decodes of the slot's previous files have read them
            jdev[:total].copy_(jpin[:total], non_blocking=True)
            slot.h2d_done.record()
        with torch.cuda.stream(slot.stream):
            slot.stream.wait_event(slot.h2d_done)
            k = 0
            for i, p in enumerate(sub):
                for side in range(2):
                    ops.jpeg_decode(jdev[offs[k]:offs[k] + len(p.data[side])], info=p.info[side], out=slot.stage[side][i], workspace=jws,
                                    status=status[srow + k:srow + k + 1])
                    k += 1
            slot.jconsumed.record()
            slot.unstage()
            slot.consumed.record()
            slot.graph.replay()
            table[row:row + len(sub)].copy_(slot.metric, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            slot.inflight.append(done)

    def run(self, dataset, groups):
        """groups: list of index lists (one forward each).  Returns a CPU fp64 [sum(len(g)), 2] table in group order."""
        self._check_weights()
        n_rows = sum(len(g) for g in groups)
        table = torch.full((max(1, n_rows), 2), float("nan"), dtype=torch.float64, device=self.device)
        status = torch.zeros((max(1, 2 * n_rows),), dtype=torch.int32, device=self.device)       # gpu_decode: one word per file
        status_paths = {}
        ready = torch.cuda.Event()
        ready.record()                                  # the slot streams write rows of `table`: after its fill
        depth = max(2 * self.nslots, self.workers)
        used = set()
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            futs = deque(pool.submit(self._load, dataset, g) for g in groups[:depth])
            nxt, row, launch = len(futs), 0, 0
            for g in groups:
                pairs, u8 = futs.popleft().result()
                if nxt < len(groups):
                    futs.append(pool.submit(self._load, dataset, groups[nxt]))
                    nxt += 1
                compressed = bool(pairs) and isinstance(pairs[0], _JpegPair)
                if compressed:
                    for sub in ([pairs] if len({p.shape for p in pairs}) == 1 else [[p] for p in pairs]):
                        H, W = sub[0].shape[:2]
                        slot = self._slot(launch % self.nslots, (len(sub), H, W), True)
                        launch += 1
                        if slot not in used:
                            slot.stream.wait_event(ready)
                            used.add(slot)
                        for j, p in enumerate(sub):
                            status_paths[2 * (row + j)], status_paths[2 * (row + j) + 1] = p.paths
                        self._launch_jpeg(slot, sub, table, row, status, 2 * row)
                        row += len(sub)
                    continue
                shapes = {p[0].shape for p in pairs} | {p[1].shape for p in pairs}
                # one forward needs one shape: a batch of mixed shapes runs pair by pair (as the plain loop does)
                for sub in ([pairs] if len(shapes) == 1 else [[p] for p in pairs]):
                    if sub[0][0].shape != sub[0][1].shape:
                        raise ValueError(f"image1 {sub[0][0].shape} and image2 {sub[0][1].shape} differ in shape")
                    H, W = (sub[0][0].shape[0:2] if u8 else sub[0][0].shape[1:3])
                    if u8 and (H * W) % 4:
                        sub, u8s = [tuple(np.ascontiguousarray(x.transpose(2, 0, 1), dtype=np.float32) for x in p) for p in sub], False
                    else:
                        u8s = u8
                    slot = self._slot(launch % self.nslots, (len(sub), H, W), u8s)
                    launch += 1
                    if slot not in used:
                        slot.stream.wait_event(ready)
                        used.add(slot)
                    self._launch(slot, sub, table, row)
                    row += len(sub)
        for slot in used:
            torch.cuda.current_stream().wait_stream(slot.stream)
            slot.inflight.clear()
        out = table[:n_rows].cpu()                     # the loop's one synchronisation
        if status_paths:
            bad = [(status_paths[j], int(v)) for j, v in enumerate(status.cpu().tolist()) if v and j in status_paths]
            if bad:
                raise RuntimeError("gpu_decode: the scan of " + ", ".join(f"{p} (status {v})" for p, v in bad) + " does not hold the frame's blocks")
        return out


def _groups(dataset, mine, batch_size):
    """consecutive runs of <= batch_size indices (the reference's DataLoader order, evaluate.py:34); batch_size 1 = one pair each."""
    return [mine[s:s + batch_size] for s in range(0, len(mine), batch_size)]


@torch.no_grad()
def validate_with_model(model, val_dataset, batch_size=1, device=None, verbose=False, pipelined=True, streams=3, decode_workers=None, gpu_decode=False):
    """Sharded evaluate.py:23-107.  Returns (result_dict, table[n_pairs, 2] of per-pair (psnr, ssim)).  gpu_decode: decode the JPEG files on
    the device (the pipelined loop only; module docstring)."""
    if gpu_decode and not pipelined:
        raise ValueError("gpu_decode belongs to the pipelined loop")
    rank, world, local = sdist.init()
    device = device or torch.device("cuda", local)
    n = len(val_dataset)
    mine = sdist.shard_indices(n, rank, world)
    if model.training:
        raise NotImplementedError("inference-only drop-in: call .eval() first")
    if pipelined:
        pipe = getattr(model, "_eval_pipeline", None)
        if pipe is None or pipe.nslots != max(1, int(streams)) or pipe.device != device:
            pipe = EvalPipeline(model, device, streams=streams, decode_workers=decode_workers)
            model._eval_pipeline = pipe
        pipe.gpu_decode = bool(gpu_decode)
        with torch.cuda.device(device):
            vals = pipe.run(val_dataset, _groups(val_dataset, mine, batch_size)).tolist() if mine else []
        if verbose:
            for i, (p, s) in zip(mine, vals):
                print(f"rank {rank}: i = {i}, psnr = {p:.6f} ssim = {s:.6f}")
    else:
        vals = []
        for idx in _groups(val_dataset, mine, batch_size):
            items = [val_dataset[i] for i in idx]
            same = len({tuple(it[0].shape) for it in items}) == 1
            groups = [items] if same else [[it] for it in items]
            for grp in groups:
                a = torch.stack([it[0] for it in grp]).to(device)
                b = torch.stack([it[1] for it in grp]).to(device)
                out = model(a, b, type="test_eval")
                m = ops.masked_psnr_ssim(a.contiguous(), out["final_warp_output"]).cpu()
                vals.extend(m.tolist())
                if verbose:
                    for (p, s) in m.tolist():
                        print(f"rank {rank}: psnr = {p:.6f} ssim = {s:.6f}")
    table = sdist.gather_metrics(mine, vals if vals else torch.zeros((0, 2)), n, k=2)
    return summarize(table[:, 0].tolist(), table[:, 1].tolist()), table
