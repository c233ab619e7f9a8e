"""Warm-started stitching of a frame sequence: every call starts FlowFormer's refinement from the forward splat of the previous
call's low-resolution flow (the reference's ``flow_init`` + ``core/utils/utils.py:32-60 forward_interpolate``), state on the device.

    seq = stitch_amd.SequenceStitcher(model, type="test_eval", graphed=True)
    for a, b in frames:
        out = seq(a, b)            # the dict of model(a, b, type="test_eval")

The state is one buffer [nB, 2, H/8, W/8] in low-resolution pixels (nB = 2B where the branch runs both flow directions as one
batch, a->b first; B where it runs one).  It is read where the decoder builds its start point (``ops.coords_grid(init=...)``) and
overwritten at the end of the call by ``ops.forward_interpolate`` of that call's final coords1: two launches on the call's stream,
no host synchronisation.  A zero state IS the cold start (grid + 0.0 == grid), so one launch sequence -- and one hipGraph --
serves every frame, and the first call after ``reset()`` equals ``model(...)`` bit for bit.  Nothing here says anything about
quality at fewer iterations: ``iters`` is a throughput knob whose effect on the flow depends on the weights.
"""
from __future__ import annotations

import torch

from . import ops


class SequenceStitcher:
    def __init__(self, model, type="test_eval", iters=None, graphed=False):
        if type not in ("test_eval", "test_out"):
            raise NotImplementedError("SequenceStitcher runs the inference paths: type='test_eval' or 'test_out'")
        if graphed and type != "test_eval":
            raise NotImplementedError("only the fixed-shape test_eval path can be captured (test_out reads its canvas size back mid-way)")
        if iters is not None and (int(iters) != iters or iters < 1):
            raise ValueError("iters must be a positive integer (None: the configured 12)")
        self.model, self.type, self.graphed = model, type, graphed
        self.iters = None if iters is None else int(iters)
        self._bufs = {}            # (shape, device) -> state buffer; kept for the object's life: captured graphs point at them
        self._cur = None
        self._graphs = {}
        self._ws = {}

    # ------------------------------------------------------------------ the state
    def buffer(self, shape, dev):
        """the state buffer of this shape on ``dev`` (created zeroed: the cold start); called by the model's flow pass"""
        key = (tuple(shape), str(dev))
        if key not in self._bufs:
            self._bufs[key] = torch.zeros(shape, device=dev)
        self._cur = key
        return self._bufs[key]

    def reset(self):
        """back to the cold start: the next call equals ``model(...)``"""
        for t in self._bufs.values():
            t.zero_()

    def state(self):
        """a copy of the next call's flow_init [nB,2,H/8,W/8] (None before the first call of a flow branch)"""
        return None if self._cur is None else self._bufs[self._cur].clone()

    def set_state(self, t):
        """overwrite the next call's flow_init (low-resolution pixels; both directions where the branch has two, a->b first)"""
        dev = next(self.model.parameters()).device
        self.buffer(tuple(t.shape), dev).copy_(t)

    # ------------------------------------------------------------------ calls
    def _workspace(self, dev):
        if str(dev) not in self._ws:
            self._ws[str(dev)] = ops.new_workspace(dev)      # this object's own split-K slabs: several sequences may run on several streams
        return self._ws[str(dev)]

    def _run(self, a, b):
        return self.model._forward(a, b, self.type, "constant", None, self)

    def __call__(self, image1, image2):
        m = self.model
        dev = next(m.parameters()).device
        if dev.type != "cuda" or not self.graphed:
            if dev.type != "cuda":
                return self._run(image1, image2)             # raises: there is no CPU path
            with ops.workspace_scope(self._workspace(dev)):
                return self._run(image1, image2)
        key = (tuple(image1.shape), dev.index, m.eval_branch(), m.sources(), self.iters)      # a cfg flip re-captures
        ent = self._graphs.get(key)
        if ent is not None and ent[4] != m.weights_generation():                 # weights re-packed since the capture
            ent = None
            self._graphs.clear()
        if ent is None:
            a = image1.to(dev).float().contiguous().clone()
            b = image2.to(dev).float().contiguous().clone()
            ws = self._workspace(dev)
            saved = {k: t.clone() for k, t in self._bufs.items()}
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), ops.workspace_scope(ws):
                for _ in range(2):                           # warm-up: weight prepack, constant tables, the state buffer itself
                    self._run(a, b)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            for k, t in self._bufs.items():                  # the warm-up runs advanced the state: put it back (new buffer: cold)
                t.copy_(saved[k]) if k in saved else t.zero_()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph), ops.workspace_scope(ws):
                out = self._run(a, b)
            ent = self._graphs[key] = (graph, a, b, out, m.weights_generation(), self._cur)
        graph, a, b, out = ent[:4]
        self._cur = ent[5]                                   # the state buffer this graph reads and writes
        a.copy_(image1)
        b.copy_(image2)
        graph.replay()
        return out
