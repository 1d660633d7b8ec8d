"""Packed self-play records -> training batches on the device, with the board's left-right mirror as augmentation.

A Xiangqi board is symmetric across the e-file: a position with its files reversed, with the same reversal applied to the
moves of its visit distribution, is an equally valid training sample (the reference does not use this; every record here can
be learnt from twice).  The mirror acts on the BOARD (b[r][f] -> b[r][8 - f]) and on the LABELS (tables()["mirror"]: a..i ->
i..a, ranks unchanged), before try_flip / unflip and the plane encoding.  The net's input planes are read with the reference's
9-stride (quirk Q1, selfplay.canonical_planes), so flipping the plane tensor is NOT a board mirror.  A mirrored record keeps its
children in the order they were generated for the unmirrored board (the generator would list the mirrored board's moves in
another order): nothing may assume generation order for it.

  mirror_records   the numpy statement on packed records: selfplay.to_dense(mirror_records(rec)) is the augmented sample
  RecordExpander   cz_records_expand (csrc/cz_records.hip): records -> (planes, pi, z) device tensors in one launch, the
                   mirror one flag per record — what train.policy_update(expand=...) builds its mini-batch with
"""
import numpy as np
import torch

from ._lib import NLABELS, NSQ, REC_BYTES, REC_COUNT, REC_LABELS, tables
from .engine import Context

RECORDS_PER_WORKGROUP = 4   # CZR_WAVES of csrc/cz_records.hip: one wave per record


def mirror_records(rec, flags=None):
    """uint8 [n, REC_BYTES] packed records -> a copy with the records whose flag is set (flags None: all of them) mirrored
    left-right: the board's files reversed and the first `count` labels mapped through tables()["mirror"].  Side, count, z,
    flags, ply, the visits and the unused label slots stay byte for byte; so does the order of the children."""
    rec = np.ascontiguousarray(rec, np.uint8).reshape(-1, REC_BYTES)
    n = rec.shape[0]
    sel = np.ones(n, bool) if flags is None else np.asarray(flags).reshape(n).astype(bool)
    out = rec.copy()
    if not sel.any():
        return out
    out[sel, :NSQ] = rec[sel, :NSQ].reshape(-1, 10, 9)[:, :, ::-1].reshape(-1, NSQ)
    lab = rec[:, REC_LABELS:REC_LABELS + 256].copy().view(np.uint16).reshape(n, 128)
    live = sel[:, None] & (np.arange(128)[None, :] < rec[:, REC_COUNT].astype(np.int64)[:, None])
    lab[live] = tables()["mirror"].astype(np.uint16)[lab[live]]
    out[:, REC_LABELS:REC_LABELS + 256] = lab.view(np.uint8).reshape(n, 256)
    return out


class RecordExpander:
    """cz_records_expand on a context of its own, or on a given one (the engine's: same device, same stream)."""

    def __init__(self, ctx=None, device=0):
        self.ctx = ctx or Context(1, 2, device)
        self.dev = self.ctx.device

    def expand(self, rec, mirror=None, temperature=1.0):
        """rec: uint8 [n, REC_BYTES] host array (uploaded in one copy) or device tensor; mirror: None, or one flag per record
        (array or tensor; non-zero = expand the record's mirror image) -> (planes [n,9,10,14] f32, pi [n,2086] f32, z [n] f32)
        device tensors: selfplay.to_dense(mirror_records(rec, mirror), temperature) with pi rounded to float32."""
        rec = self.ctx.tensor(rec, torch.uint8).reshape(-1, REC_BYTES)
        n = rec.shape[0]
        flags = self.ctx.tensor(mirror, torch.uint8)
        if flags is not None and flags.numel() != n:
            raise ValueError("RecordExpander.expand: %d mirror flags for %d records" % (flags.numel(), n))
        planes = torch.empty((n, 9, 10, 14), dtype=torch.float32, device=self.dev)
        pi = torch.empty((n, NLABELS), dtype=torch.float32, device=self.dev)
        z = torch.empty(n, dtype=torch.float32, device=self.dev)
        self.ctx.call("cz_records_expand", rec, n, flags, float(temperature), planes, pi, z)
        return planes, pi, z

    __call__ = expand
