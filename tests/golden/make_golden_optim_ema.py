"""Generates tests/golden/optim_ema.npz by running the REFERENCE's ModelEma (/root/reference/utils/ema_utils.py) on `small_module()`:
for world sizes 1, 2 and 8 and every rank, the rank's shard of names (`names`) and the keys of its `shadow`.  The class reads
rank / world size from torch.distributed only in its constructor, so the shards of a several-rank run are made here without a process
group: an instance is created without the constructor, rank and world_size are set by hand and `register()` is called.
Runs in the build container only (needs /root/reference); the fixture it writes is data: arrays of names, and the shadow values of the
one-rank run (which are the module's parameters)."""
import importlib.util
import os

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
WORLD_SIZES = (1, 2, 8)


def small_module() -> nn.Module:
    """Parameters and buffers at several depths; names that sort differently from their registration order."""
    torch.manual_seed(7)

    class Block(nn.Module):
        def __init__(self, c):
            super().__init__()
            self.conv = nn.Linear(c, c)
            self.norm = nn.BatchNorm1d(c)
            self.register_buffer("anchor", torch.arange(c, dtype=torch.float32))

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = nn.Linear(5, 8, bias=False)
            self.blocks = nn.ModuleList([Block(8), Block(8)])
            self.head = nn.Sequential(nn.Linear(8, 8), nn.LayerNorm(8), nn.Linear(8, 3))
            self.scale = nn.Parameter(torch.ones(3))
            self.register_buffer("a_table", torch.zeros(2, 2))

    return Net()


def main():
    spec = importlib.util.spec_from_file_location("ref_ema", "/root/reference/utils/ema_utils.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for world in WORLD_SIZES:
        for rank in range(world):
            ema = ref.ModelEma.__new__(ref.ModelEma)
            ema.model, ema.decay, ema.shadow, ema.backup, ema.rank, ema.world_size = small_module(), 0.9997, {}, {}, rank, world
            ema.register()
            out[f"names_w{world}_r{rank}"] = np.array(ema.names, dtype=str)
            out[f"shadow_keys_w{world}_r{rank}"] = np.array(list(ema.shadow.keys()), dtype=str)
            if world == 1:
                for k, v in ema.shadow.items():
                    out[f"shadow_value/{k}"] = v.numpy()
    np.savez_compressed(os.path.join(HERE, "optim_ema.npz"), **out)
    print("wrote optim_ema.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
