"""Ragged batches on the host, for the command-line tools: which items go into which batch (`plan_batches`) and the zero-padded
tensor of one batch with its lengths (`pad_batch`)."""
from __future__ import annotations

import torch

__all__ = ["plan_batches", "pad_batch"]


def plan_batches(lengths, max_batch: int, max_padded=None):
    """Cut items of the given lengths into batches: -> a list of lists of indices into `lengths`.  The items are sorted by length (ties in
    index order) and taken in that order; a batch is closed when one more would make it larger than `max_batch` items or, with
    `max_padded`, its padded size (items x its longest) larger than that.  Every index appears exactly once; an item that alone is larger
    than `max_padded` gets a batch of its own.  Lengths are checked (at least 1, the item named) only when `max_padded` is given."""
    if max_batch < 1 or (max_padded is not None and max_padded < 1):
        raise ValueError("plan_batches: max_batch and max_padded must be at least 1")
    order = sorted(range(len(lengths)), key=lambda i: (int(lengths[i]), i))
    if max_padded is None:
        return [order[i:i + max_batch] for i in range(0, len(order), max_batch)]
    batches, cur = [], []
    for i in order:
        n = int(lengths[i])                      # ascending: the newcomer is the longest of the batch it joins
        if n < 1:
            raise ValueError(f"plan_batches: utterance {i} has length {n}")
        if cur and (len(cur) + 1 > max_batch or (len(cur) + 1) * n > max_padded):
            batches.append(cur)
            cur = []
        cur.append(i)
    if cur:
        batches.append(cur)
    return batches


def pad_batch(items):
    """1-D tensors or arrays of one dtype -> (x [B, longest] of that dtype, zero beyond each item, on the items' device (the host for
    arrays); the lengths as a list)."""
    items = [torch.as_tensor(v) for v in items]
    n = [int(v.shape[0]) for v in items]
    x = torch.zeros(len(items), max(n), dtype=items[0].dtype, device=items[0].device)
    for b, v in enumerate(items):
        x[b, :n[b]] = v
    return x, n
