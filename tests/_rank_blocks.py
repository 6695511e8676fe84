"""One rank of the multi-process error-block test (started by semiclassical_amd.distributed.launch_local_ranks).

Every rank runs the HIP engine on ITS shard of a golden case's initial conditions on cuda:0 with the global N as Monte-Carlo
weight and blocks on (the shard is partitioned by the rank-local index), flushes slots, blocks and block counts through
distributed.flush_correlations (gloo: one all-reduce of all three) and rank 0 stores the flushed buffers.

    python tests/_rank_blocks.py CASE NT B OUT.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch.set_default_dtype(torch.float64)


def main():
    case, nt, nblocks, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    import torch.distributed as dist
    from semiclassical_amd import distributed as D
    from tests import cases
    from tests.engine_cases import engine_potential, engine_propagator
    rank, world, _ = D.init_from_env()
    dev = torch.device("cuda", int(os.environ.get("SC_TEST_DEVICE", "0")))
    torch.cuda.set_device(dev)
    g = cases.load(case)
    n_total = g["zi"].shape[1]
    prop = engine_propagator(g, device=dev, select=D.shard_slice(n_total, rank, world), ntraj_total=n_total)
    slots = torch.zeros((nt, 5), dtype=torch.float64, device=dev)
    blocks = torch.zeros((nt, nblocks, 4), dtype=torch.float64, device=dev)
    counts = torch.from_numpy(prop.block_counts(prop.ntraj, nblocks)).to(torch.float64)
    prop.run(engine_potential(g), float(g["dt"]), nt, float(g["E0"]), slots=slots, blocks=blocks)
    calls = []
    real = dist.all_reduce

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    dist.all_reduce = counted
    D.flush_correlations(slots, None, blocks, counts)
    dist.all_reduce = real
    prop.synchronize()
    if rank == 0:
        np.savez(out, slots=slots.cpu().numpy(), blocks=blocks.cpu().numpy(), counts=np.rint(counts.numpy()).astype(np.int64),
                 world=world, collectives=len(calls))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
