"""The one way the learner enters libmapdn_hip.so (C ABI: include/mapdn.h, argument types: mapdn_amd/_lib.py).  Loaded on first use."""

import torch

from .. import _lib


def entry(name: str):
    """lib.<name> for the calls that are no launch (mapdn_policy_forward_fits, mapdn_critic_shapley_geometry)"""
    return getattr(_lib.load(), name)


def launch(name: str, dev, *args) -> None:
    """lib.<name>(*args, stream) on `dev` and its current stream, checked.  A tensor goes in as its data pointer, None as NULL, numbers as
    they are.  Tensors must be contiguous already: what is copied, cast or detached — and so what is saved for backward — stays with the caller."""
    assert all(a.is_contiguous() for a in args if torch.is_tensor(a)), name
    ptrs = [a.data_ptr() if torch.is_tensor(a) else a for a in args]
    with torch.cuda.device(dev):
        _lib.check(entry(name)(*ptrs, torch.cuda.current_stream(dev).cuda_stream))


def buffer(name: str, dev, *dims, per: int = 1, at_least: int = 0) -> torch.Tensor:
    """an uninitialised f32 buffer on `dev` of max(at_least, lib.<name>(*dims) * per) elements, for the size queries (mapdn_*_scratch_floats,
    mapdn_layernorm64_backward_blocks, mapdn_ppo_loss_blocks).  Their block counts follow the CU count of the CURRENT device: asked inside
    the device context."""
    with torch.cuda.device(dev):
        return torch.empty(max(at_least, entry(name)(*dims) * per), dtype=torch.float32, device=dev)
