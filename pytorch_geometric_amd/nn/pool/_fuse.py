"""The route switch of the hierarchical pooling layers and functions, and their defaults.

``PYGAMD_FUSE_POOL`` (read at import): ``0`` / ``1`` start ``TopKPooling``, ``SAGPooling``,
``topk`` and ``filter_adj`` with the kernels of csrc/pool.hip off / on.  Unset, each starts with
what was measured for it (profiles/hier_pool.md): ``DEFAULTS`` below."""
import os

import torch

_SWITCH = os.environ.get('PYGAMD_FUSE_POOL')
FUSE_POOL = None if _SWITCH is None else _SWITCH.strip() not in ('', '0')

# forward + backward of the layer, fused against generic, at the three shapes of
# scripts/time_pool.py; the two functions follow the layers they serve
DEFAULTS = {'TopKPooling': True, 'SAGPooling': True, 'topk': True, 'filter_adj': True}

LOW = (torch.float16, torch.bfloat16)   # widened to float32 around the kernels


def fuse_default(what: str) -> bool:
    """the initial ``fuse`` of ``what`` (a key of ``DEFAULTS``)"""
    return DEFAULTS[what] if FUSE_POOL is None else FUSE_POOL
