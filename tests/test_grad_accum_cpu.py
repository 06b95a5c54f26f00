"""CPU: the host side of gradient accumulation -- `mobi_accum_multi`'s argument checks (nothing launches), the accumulator's
bucket layout (`dist.gradient_bucket_layout`) and the once-per-window collective (`dist.allreduce_accumulated`) with world_size 2
on gloo.  The kernel and `train.GradAccumulator` are tests/test_gpu_grad_accum.py."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_dist_cpu import _free_port


def test_argument_errors_return_before_any_launch():
    from mobi_amd import _lib
    lib = _lib.load()
    assert (_lib.MT_ACCUM, _lib.MT_ASSIGN) == (0, 1)
    assert lib.mobi_abi_version() == 6 and "mobi_accum_multi" in _lib.SYMBOLS
    assert lib.mobi_accum_multi(None, 1, 16, 1, 0.5, _lib.MT_ACCUM, None) == -1
    assert lib.mobi_accum_multi(16, 1, None, 1, 0.5, _lib.MT_ASSIGN, None) == -1
    assert lib.mobi_accum_multi(16, 0, 16, 1, 0.5, _lib.MT_ACCUM, None) == -1
    assert lib.mobi_accum_multi(16, 1, 16, 0, 0.5, _lib.MT_ASSIGN, None) == -1
    assert lib.mobi_accum_multi(16, -1, 16, -1, 0.5, _lib.MT_ACCUM, None) == -1
    assert lib.mobi_accum_multi(16, 1, 16, 1, 0.5, 2, None) == -1 and lib.mobi_accum_multi(16, 1, 16, 1, 0.5, -1, None) == -1


# name -> numel: sizes that are no multiple of 4 (padding), one tensor larger than the bucket, names given out of order
NUMELS = {"m.z.weight": 700, "m.a.weight": 1001, "m.a.bias": 13, "m.k.weight": 1200, "bbox_uncond_vector": 3,
          "m.c.weight": 999, "m.b.bias": 1, "m.zz.weight": 2500, "m.r.bias": 6}
BUCKET_BYTES = 8192


def _cuts_of_allreduce_gradients(numels, bucket_bytes):
    """The bucket walk of `dist.allreduce_gradients`, restated on sizes alone: [[name]] per bucket."""
    names, out, i = sorted(numels), [], 0
    while i < len(names):
        bucket, size = [], 0
        while i < len(names) and (not bucket or size + numels[names[i]] * 4 <= bucket_bytes):
            bucket.append(names[i])
            size += numels[names[i]] * 4
            i += 1
        out.append(bucket)
    return out


@pytest.mark.parametrize("bucket_bytes", [BUCKET_BYTES, 4, 256 << 20])
def test_layout_is_sorted_aligned_and_cut_like_the_collective(bucket_bytes):
    from mobi_amd.dist import gradient_bucket_layout
    layout, lengths = gradient_bucket_layout(NUMELS, bucket_bytes)
    assert list(layout) == sorted(NUMELS) and all(layout[k][2] == NUMELS[k] for k in NUMELS)
    cuts = _cuts_of_allreduce_gradients(NUMELS, bucket_bytes)
    if bucket_bytes == BUCKET_BYTES:
        assert len(cuts) == 3 and any(NUMELS[b[0]] * 4 > bucket_bytes for b in cuts)     # (one tensor exceeds the bucket alone)
    assert len(lengths) == len(cuts)
    assert [[k for k in sorted(NUMELS) if layout[k][0] == b] for b in range(len(lengths))] == cuts
    for b, names in enumerate(cuts):
        end = 0
        for k in names:                                # in name order, 16-byte aligned, inside the bucket, never overlapping
            _, off, n = layout[k]
            assert off % 4 == 0 and end <= off < end + 4 and off + n <= lengths[b], k
            end = off + n
        assert lengths[b] % 4 == 0 and end <= lengths[b] < end + 4
    # pure and order-independent
    assert gradient_bucket_layout(dict(reversed(list(NUMELS.items()))), bucket_bytes) == (layout, lengths)


SEEN = {0: ["m.a.weight", "m.a.bias", "m.b.bias", "m.c.weight", "m.k.weight", "m.zz.weight", "m.z.weight"],   # "the embedder"
        1: ["bbox_uncond_vector", "m.k.weight", "m.zz.weight", "m.z.weight"]}
NEVER = "m.r.bias"


def _window_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mobi_amd import dist as md
    layout, lengths = md.gradient_bucket_layout(NUMELS, BUCKET_BYTES)
    ok = len(lengths) == 3

    def values(r):
        g = torch.Generator().manual_seed(200 + r)
        return {k: torch.randn(NUMELS[k], generator=g) for k in sorted(NUMELS)}
    buckets = [torch.full((n,), float("nan")) for n in lengths]       # unseen regions (and the padding) hold nan
    for k in SEEN[rank]:
        b, off, n = layout[k]
        buckets[b][off:off + n] = values(rank)[k]
    ptrs = [t.data_ptr() for t in buckets]
    present = md.allreduce_accumulated(buckets, layout, set(SEEN[rank]))
    everyone = sorted(set(SEEN[0]) | set(SEEN[1]))
    ok = ok and present == everyone and NEVER not in present
    ok = ok and [t.data_ptr() for t in buckets] == ptrs               # reduced in place
    # the same per-rank values (zeros where unseen) through today's collective, cut into the same buckets
    today = md.allreduce_gradients({k: (values(rank)[k].clone() if k in SEEN[rank] else torch.zeros(NUMELS[k])) for k in everyone},
                                   bucket_bytes=BUCKET_BYTES)
    for k in everyone:
        b, off, n = layout[k]
        got = buckets[b][off:off + n]
        ok = ok and bool(torch.isfinite(got).all()) and torch.equal(got.view(torch.int32), today[k].view(torch.int32))
    b, off, n = layout[NEVER]
    ok = ok and bool(torch.isnan(buckets[b][off:off + n]).all())      # nobody saw it: not zero-filled, not returned
    try:                                                              # a name outside the layout is an error before any collective
        md.allreduce_accumulated(buckets, layout, {"nowhere"})
        ok = False
    except ValueError:
        pass
    q.put((rank, bool(ok), present))
    dist.destroy_process_group()


def test_window_collective_gloo_world2():
    """Rank 0 saw the embedder's names, rank 1 `bbox_uncond_vector`, nobody `m.r.bias`: both ranks return the same present set,
    every present tensor is bit-equal to `allreduce_gradients` on the same values, the buffers are the ones passed in."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_window_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res), res
    assert res[0][2] == res[1][2] and NEVER not in res[0][2]


def test_single_process_makes_no_collective():
    from mobi_amd import dist as md
    layout, lengths = md.gradient_bucket_layout(NUMELS, BUCKET_BYTES)
    buckets = [torch.full((n,), 2.0) for n in lengths]
    assert md.allreduce_accumulated(buckets, layout, {"m.z.weight", "m.a.bias"}) == ["m.a.bias", "m.z.weight"]
    assert all(bool((t == 2.0).all()) for t in buckets)
