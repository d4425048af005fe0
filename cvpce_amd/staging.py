"""Host-side staging shared by the `device_*` glue: ragged per-image inputs -> packed device tensors.  Every upload goes through
pinned memory and is queued on the current stream -- the host does not wait.  Host-only: torch alone, importable without the HIP
library.
"""
import torch


def offsets(lengths):
    """[n0, n1, ...] -> [0, n0, n0 + n1, ...]: the row offsets of a packed layout"""
    off = [0]
    for n in lengths:
        off.append(off[-1] + n)
    return off


def upload(host, device):
    """A host tensor -> device tensor: pinned (unless empty), one asynchronous copy."""
    return (host.pin_memory() if host.numel() else host).to(device, non_blocking=True)


def upload_values(values, dtype, device):
    """A short host list -> device tensor, by `upload`."""
    return upload(torch.tensor(values, dtype=dtype), device)


def pack(tensors, dtype, device, tail=()):
    """Per-image tensors (device or host) -> one packed device tensor; one upload per host tensor."""
    if not tensors:
        return torch.zeros((0,) + tail, dtype=dtype, device=device)
    parts = []
    for t in tensors:
        t = t.detach().reshape((-1,) + tail)
        if not t.is_cuda:
            t = t.to(dtype)
            t = t.pin_memory() if t.numel() else t
        parts.append(t.to(device=device, dtype=dtype, non_blocking=True))
    return torch.cat(parts) if len(parts) > 1 else parts[0].contiguous()


def pack_once(tensors, dtype, device, tail=()):
    """Per-image host tensors -> packed on the host, ONE upload; with a device tensor among them, `pack`."""
    if any(t.is_cuda for t in tensors):
        return pack(tensors, dtype, device, tail)
    host = torch.cat([t.detach().reshape((-1,) + tail).to(dtype) for t in tensors])
    if not host.numel():
        return torch.empty((0,) + tail, dtype=dtype, device=device)
    return upload(host, device)
