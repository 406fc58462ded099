"""GPU: two growth edges of the context's scratch that no other test forces, each on a fresh DeviceCodec.

1. The per-launch table of the compress from device tables starts at 16 entries (tsqa_ctx::reserve_tables).  A call with
   cap_blocks = 16 * budget + 1 takes 17 launches, all but the first dead, and grows it to 32 between two calls that take one.
2. The frame descriptors are reallocated (1 -> 2 blocks) by a plain decompress behind a sharded fetch + decode: what that call left
   for tsqa_sharded_decode_again_async goes with them.

Neither test races a growth against running kernels: every call here is waited for before the next one starts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_OVERFLOW = 0, 3, 6
ALIGN = 16


def sentinel(n):
    """((i * 37 + 11) % 251) ^ 0xA5 at byte i (test_gpu_dense.py's pattern)"""
    return np.resize(((np.arange(251, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5, n)


@pytest.fixture(scope="module")
def tsq():
    import torch
    assert torch.cuda.is_available()
    import turbosqueeze_amd
    return turbosqueeze_amd


def test_launch_table_grows_past_its_first_size(tsq, oracle):
    """Three items of a few hundred bytes, one block each.  cap_blocks = 1 admits the first alone (the other two: TSQA_ERR_OVERFLOW,
    size 0); cap_blocks = 16 * budget + 1 admits all three.  So the third call must give what the first gave, to the byte, the
    second must place the first item where they do, and every admitted item's container is the oracle's."""
    import torch
    budget = 2 * torch.cuda.get_device_properties(0).multi_processor_count     # (as test_gpu_compress_tables.py takes it)
    lens = [300, 517, 411]
    at = [0, 300, 817]
    host = tsq.synth.text(sum(lens), seed=21)[:sum(lens)].copy()
    want = [oracle.compress(host[a:a + n], 1, threads=1) for a, n in zip(at, lens)]
    data = torch.from_numpy(host).cuda()
    d_at, d_len = torch.tensor(at, dtype=torch.int64, device="cuda"), torch.tensor(lens, dtype=torch.int64, device="cuda")
    c = tsq.DeviceCodec(0)
    try:
        def call(cap_blocks):
            out = torch.from_numpy(sentinel(1 << 16)).cuda()
            pb, status = c.compress_packed_tables(data, d_at, d_len, 1, ALIGN, cap_blocks, out, item_status=True)
            for i, st in enumerate(status):
                if st == OK:
                    assert pb.views[i].cpu().numpy().tobytes() == want[i], f"cap_blocks {cap_blocks}: item {i} differs from the oracle's container"
                else:
                    assert pb.sizes[i] == 0
            return dict(arena=out.cpu().numpy().tobytes(), offsets=pb.offsets, sizes=pb.sizes, status=status)

        first = call(1)
        assert first["status"] == [OK, ERR_OVERFLOW, ERR_OVERFLOW] and first["sizes"][0] == len(want[0])
        wide = call(16 * budget + 1)                                 # 17 launches: the launch table grows, 16 -> 32 entries
        assert wide["status"] == [OK] * 3 and wide["sizes"] == [len(w) for w in want]
        places, end = [], 0
        for w in want:                                               # (tsqa_plan_packed: each item at the next multiple of align)
            places.append((end + ALIGN - 1) // ALIGN * ALIGN)
            end = places[-1] + len(w)
        assert wide["offsets"] == places + [end]
        assert wide["offsets"][0] == first["offsets"][0]
        again = call(1)
        assert again == first
    finally:
        c.close()


def test_regrown_descriptors_forget_the_sharded_decode(tsq):
    """Both containers come from another context, so that the context under test sees one block (the sharded call), then two (the
    plain decompress: 4 MiB + 1 byte), and nothing else."""
    import torch
    n1, n2 = 5000, tsq.BLOCK_SZ + 1
    host = tsq.synth.text(n2, seed=33)[:n2].copy()
    src = torch.from_numpy(host).cuda()
    maker = tsq.DeviceCodec(0)
    try:
        blob1 = maker.compress(src[:n1], 0).cpu().numpy().copy()
        blob2 = maker.compress(src, 0).clone()
    finally:
        maker.close()
    fill = torch.from_numpy(sentinel(tsq.BLOCK_SZ)).cuda()
    c = tsq.DeviceCodec(0)
    try:
        streams = torch.empty(tsq.OUTPUT_SZ, dtype=torch.uint8, device="cuda")
        out = fill.clone()
        assert c.sharded_fetch_decode_async(blob1.ctypes.data, len(blob1), 0, 1, streams, out) == n1
        torch.cuda.synchronize()
        assert c.status() == 0 and torch.equal(out[:n1], src[:n1]) and torch.equal(out[n1:], fill[n1:])
        out.copy_(fill)
        back = c.decompress(blob2)                                   # the descriptors grow from one block to two
        torch.cuda.synchronize()
        assert torch.equal(back, src)
        with pytest.raises(tsq.TsqError) as e:
            c.sharded_decode_again_async(streams, out)
        assert e.value.code == ERR_ARG, e.value
        torch.cuda.synchronize()
        assert torch.equal(out, fill)
    finally:
        c.close()
