"""world_size-2 gloo tests (CPU) of the N>1 path: window sharding, bank broadcast from the owning
rank, and re-assembly.  The per-window compute is the CPU oracle here (the HIP path needs a GPU);
what is under test is that a sharded run reproduces the single-process result."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from mocha_sigasia2023_amd import distributed as D
from mocha_sigasia2023_amd import synthetic, weights
from oracle import mocha_oracle as O

N_SRC, N_CHA = 5, 4
# Every process computes at this thread count: with another, MKL / oneDNN may split a reduction differently and the last bit moves
# (seen on AVX2 code paths), so bit-for-bit comparisons hold only between computations at the same count.
THREADS = 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _bank_and_decode(sd, src, bank_nm, bank_enc, mean, std):
    enc, cnt = O.encode(sd, src)
    idx, _ = O.match_bruteforce(O.znorm(cnt.numpy(), mean, std), bank_nm.numpy())
    Y = O.to_mot(sd, O.decoder(sd, enc, bank_enc[torch.from_numpy(idx)]))
    return Y, torch.from_numpy(idx)


def _worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(THREADS)
    D.init("gloo")
    sd = O.to_torch_state(weights.synthetic_state_dict(5, 1.0))
    mean, std = synthetic.cnt_norm(3)
    src_all = torch.from_numpy(synthetic.pose_windows(10, N_SRC))
    with torch.no_grad():
        # rank 0 owns the character clip and builds the bank; the others receive it
        if rank == 0:
            enc_c, cnt_c = O.encode(sd, torch.from_numpy(synthetic.pose_windows(11, N_CHA)))
            bank_enc = enc_c.contiguous()
            bank_nm = torch.from_numpy(O.znorm(cnt_c.numpy(), mean, std)).contiguous()
        else:
            bank_enc = torch.empty((N_CHA, 90, 256))
            bank_nm = torch.empty((N_CHA, 90, 256))
        D.broadcast_([bank_nm, bank_enc], src=0)
        np.save(os.path.join(out_dir, f"bank_nm_rank{rank}.npy"), bank_nm.numpy())      # what every rank holds after the broadcast
        lo, hi = D.shard_bounds(N_SRC, world, rank)
        Y, idx = _bank_and_decode(sd, src_all[lo:hi], bank_nm, bank_enc, mean, std)
        Y_all = D.all_gather_rows(Y, N_SRC)
        idx_all = D.all_gather_rows(idx, N_SRC)
        t = D.max_over_ranks(float(rank + 1), torch.device("cpu"))
    D.barrier()
    if rank == 0:
        np.savez(os.path.join(out_dir, "dist.npz"), Y=Y_all.numpy(), idx=idx_all.numpy(), t=t,
                 bank_nm=bank_nm.numpy())
    torch.distributed.destroy_process_group()


def test_shard_bounds_cover_everything():
    for n in (0, 1, 7, 585, 1024):
        for world in (1, 2, 3, 8):
            spans = [D.shard_bounds(n, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1
    assert D.shard_bounds(1024, 8, 3) == (384, 512)          # BASELINE configs[3]: 128 windows per GPU


@pytest.mark.timeout(600)
def test_two_rank_run_matches_single_process(tmp_path):
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    z = np.load(tmp_path / "dist.npz")
    # single-process reference, at the ranks' thread count
    sd = O.to_torch_state(weights.synthetic_state_dict(5, 1.0))
    mean, std = synthetic.cnt_norm(3)
    before = torch.get_num_threads()
    torch.set_num_threads(THREADS)
    try:
        with torch.no_grad():
            enc_c, cnt_c = O.encode(sd, torch.from_numpy(synthetic.pose_windows(11, N_CHA)))
            bank_nm = torch.from_numpy(O.znorm(cnt_c.numpy(), mean, std))
            Y, idx = _bank_and_decode(sd, torch.from_numpy(synthetic.pose_windows(10, N_SRC)), bank_nm, enc_c, mean, std)
    finally:
        torch.set_num_threads(before)
    assert np.array_equal(np.load(tmp_path / "bank_nm_rank1.npy"), z["bank_nm"])     # the broadcast bank is the owner's bank
    assert np.array_equal(z["bank_nm"], bank_nm.numpy())          # ... and the owner's bank is the single-process one
    assert np.array_equal(z["idx"], idx.numpy())                  # shards are independent: same matches
    assert np.abs(z["Y"] - Y.numpy()).max() < 1e-5                # oneDNN blocking differs with batch size: ~1e-7
    assert float(z["t"]) == 2.0                                   # max over ranks
