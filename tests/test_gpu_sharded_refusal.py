"""GPU: a sharded fetch + decode that refuses its container leaves nothing for tsqa_sharded_decode_again_async to repeat -- the
descriptors of the context's previous sharded decode are forgotten before the first check, whichever check refuses."""
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_FORMAT = 3, 4


@pytest.mark.parametrize("damage", ["bad-magic", "streams-too-small"])
def test_refused_fetch_forgets_the_previous_decode(damage):
    import torch
    import turbosqueeze_amd as tsq
    n = tsq.BLOCK_SZ + 5000
    src = torch.from_numpy(tsq.synth.text(n, seed=7)[:n].copy()).cuda()
    c = tsq.DeviceCodec(0)
    try:
        blob = c.compress(src, 0).cpu().numpy().copy()
        streams = torch.empty(2 * tsq.OUTPUT_SZ, dtype=torch.uint8, device="cuda")
        out = torch.zeros(2 * tsq.BLOCK_SZ, dtype=torch.uint8, device="cuda")
        assert c.sharded_fetch_decode_async(blob.ctypes.data, len(blob), 0, 1, streams, out) == n
        c.sharded_decode_again_async(streams, out)                   # the last call's descriptors may be decoded again ...
        torch.cuda.synchronize()
        assert c.status() == 0 and torch.equal(out[:n], src)
        bad, bad_streams = blob.copy(), streams
        if damage == "bad-magic":
            bad[0] ^= 0xFF
        else:
            bad_streams = streams[:tsq.OUTPUT_SZ]                    # two owned frames do not fit
        with pytest.raises(tsq.TsqError) as e:
            c.sharded_fetch_decode_async(bad.ctypes.data, len(bad), 0, 1, bad_streams, out)
        assert e.value.code == ERR_FORMAT, e.value
        with pytest.raises(tsq.TsqError) as e:                       # ... but not once a later call has refused its container
            c.sharded_decode_again_async(streams, out)
        assert e.value.code == ERR_ARG, e.value
        torch.cuda.synchronize()
    finally:
        c.close()
