"""The device plumbing every GPU-resident class repeats: which device, which stream, which pointer."""

U64 = 0xFFFFFFFFFFFFFFFF  # seeds, draws and step indices cross the C ABI as uint64


def require_gpu(name):
    """torch, or the RuntimeError of class `name`, which has no CPU fallback."""
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError(f"{name} needs a ROCm GPU; there is no CPU fallback")
    return torch


def cuda_device(torch, device, default=None):
    """torch.device of `device` (None: `default`, else "cuda"), an index-less one resolved to the current device."""
    dev = torch.device(device if device is not None else default if default is not None else "cuda")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def raw_stream(torch, device):
    """Raw handle of torch's current stream on `device` (honours `torch.cuda.stream(...)`)."""
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    """t.data_ptr(), or None (a NULL argument) for None."""
    return None if t is None else t.data_ptr()
