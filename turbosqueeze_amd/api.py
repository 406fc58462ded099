"""ctypes binding of libturbosqueeze_amd.so (include/turbosqueeze_amd.h).

Two faces:
  * DeviceCodec  -- tsqa_* device-resident entry points over torch CUDA(HIP) tensors.
    torch is used only for device memory and streams.
  * tsq_encode / tsq_decode / tsq_compress_mt / tsq_decompress_mt -- the reference's own
    API names (turbosqueeze.h:508,580,657,670) over host bytes, same argument meaning.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK_SZ = 1 << 22
OUTPUT_SZ = BLOCK_SZ + (BLOCK_SZ >> 2)

ERRORS = {1: "no usable gfx950 device", 2: "HIP runtime error", 3: "bad argument", 4: "malformed container",
          5: "malformed block stream", 6: "block expanded beyond TSQ_OUTPUT_SZ",
          7: "multi-workgroup decode stalled waiting for a sibling workgroup (the container may be fine: decode again with variant 4)"}


class TsqError(RuntimeError):
    def __init__(self, code: int, detail: str = ""):
        self.code = code
        super().__init__(f"turbosqueeze_amd error {code} ({ERRORS.get(code, '?')}) {detail}".strip())


def lib_path(ab=False) -> str:
    """The product library; ab=True: the A/B library that also carries the superseded kernel generations
    (`make -C turbosqueeze_amd/csrc ab`); ab="jitter": the hand-off stress build of the encoder (`make jitter`)."""
    if isinstance(ab, str):
        return os.path.join(HERE, f"libturbosqueeze_amd_{ab}.so")
    return os.path.join(HERE, "libturbosqueeze_amd_ab.so" if ab else "libturbosqueeze_amd.so")


def build_native(force: bool = False) -> None:
    """Compile every HIP source for gfx950 into turbosqueeze_amd/*.so (in-tree)."""
    csrc = os.path.join(HERE, "csrc")
    args = ["make", "-C", csrc, "all", "ab", "jitter"]
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(args, stdout=subprocess.DEVNULL)


def source_fingerprint() -> str:
    """Hash of the kernel and host sources the native libraries are built from (csrc/*.cuh, *.hip, *.h, ab/*): what a stored
    profile must carry to be attributed to the code that is running (bench.py: roofline.traffic)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(HERE, "csrc")
    for fn in sorted(glob.glob(os.path.join(csrc, "*.cuh")) + glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")) +
                     glob.glob(os.path.join(csrc, "ab", "*.cuh"))):
        h.update(os.path.basename(fn).encode())
        h.update(open(fn, "rb").read())
    return h.hexdigest()[:16]


def build_info(ab=False) -> str:
    """tsqa_build_info() of a library: which experiment / instrumentation switches it was compiled with (the product: none)."""
    return lib(ab).tsqa_build_info().decode()


_libs = {}


def lib(ab=False) -> C.CDLL:
    """Load the native library.  Fails loudly when it is missing: there is no other path."""
    if ab in _libs:
        return _libs[ab]
    path = lib_path(ab)
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); turbosqueeze_amd has no CPU fallback")
    L = C.CDLL(path)
    vp, u8pp, szp = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
    L.tsqa_create.restype = C.c_int
    L.tsqa_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.tsqa_destroy.restype = None
    L.tsqa_destroy.argtypes = [vp]
    L.tsqa_last_error.restype = C.c_char_p
    L.tsqa_last_error.argtypes = [vp]
    L.tsqa_device_id.restype = C.c_int
    L.tsqa_device_id.argtypes = [vp]
    L.tsqa_block_count.restype = C.c_size_t
    L.tsqa_block_count.argtypes = [C.c_size_t]
    L.tsqa_build_info.restype = C.c_char_p
    L.tsqa_build_info.argtypes = []
    L.tsqa_container_bound.restype = C.c_size_t
    L.tsqa_container_bound.argtypes = [C.c_size_t]
    L.tsqa_compress_device.restype = C.c_int
    L.tsqa_compress_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, szp, C.c_uint32, vp]
    L.tsqa_compress_device_async.restype = C.c_int
    L.tsqa_compress_device_async.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp, C.c_uint32, vp]
    L.tsqa_decompress_device.restype = C.c_int
    L.tsqa_decompress_device.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, szp, vp]
    L.tsqa_decompress_device_async.restype = C.c_int
    L.tsqa_decompress_device_async.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, C.c_size_t, vp, vp, vp]
    L.tsqa_profile_enable.restype = C.c_int
    L.tsqa_profile_enable.argtypes = [vp, C.c_int]
    L.tsqa_profile_read.restype = C.c_int
    L.tsqa_profile_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.tsqa_set_kernel_variant.restype = None
    L.tsqa_set_kernel_variant.argtypes = [vp, C.c_int, C.c_int]
    L.tsqa_set_decode_wait_limit.restype = None
    L.tsqa_set_decode_wait_limit.argtypes = [vp, C.c_uint32]
    # reference API
    L.tsqAllocateContext.restype = vp
    L.tsqDeallocateContext.argtypes = [vp]
    L.tsqInit.argtypes = [vp]
    L.tsqEncode.restype = None
    L.tsqEncode.argtypes = [vp, vp, vp, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32]
    L.tsqDecode.restype = None
    L.tsqDecode.argtypes = [vp, vp, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32]
    L.tsqAllocateContextCompression_MT.restype = vp
    L.tsqAllocateContextCompression_MT.argtypes = [C.c_bool]
    L.tsqDeallocateContextCompression_MT.argtypes = [vp]
    L.tsqAllocateContextDecompression_MT.restype = vp
    L.tsqAllocateContextDecompression_MT.argtypes = [C.c_bool]
    L.tsqDeallocateContextDecompression_MT.argtypes = [vp]
    L.tsqCompress_MT.restype = C.c_bool
    L.tsqCompress_MT.argtypes = [vp, vp, C.c_size_t, C.c_bool, u8pp, szp, C.c_bool, C.c_bool, C.c_uint32]
    L.tsqDecompress_MT.restype = C.c_bool
    L.tsqDecompress_MT.argtypes = [vp, vp, C.c_size_t, C.c_bool, u8pp, szp, C.c_bool]
    L.tsqa_compress_async_cb.restype = C.c_uint32
    L.tsqa_compress_async_cb.argtypes = [vp, vp, C.c_size_t, C.c_bool, u8pp, szp, C.c_bool, C.c_bool, C.c_uint32, vp, vp, vp]
    L.tsqa_decompress_async_cb.restype = C.c_uint32
    L.tsqa_decompress_async_cb.argtypes = [vp, vp, C.c_size_t, C.c_bool, u8pp, szp, C.c_bool, vp, vp, vp]
    L.tsqa_profile_read_calls.restype = C.c_int
    L.tsqa_profile_read_calls.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.tsqa_profile_read_join.restype = C.c_int
    L.tsqa_profile_read_join.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.tsqa_encode_blocks_async.restype = C.c_int
    L.tsqa_encode_blocks_async.argtypes = [vp, vp, C.c_uint32, C.c_size_t, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.tsqa_decode_blocks_async.restype = C.c_int
    L.tsqa_decode_blocks_async.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, vp]
    L.tsqa_frames_to_host_async.restype = C.c_int
    L.tsqa_frames_to_host_async.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp]
    L.tsqa_frames_from_host_async.restype = C.c_int
    L.tsqa_frames_from_host_async.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, vp]
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.tsqa_frame_offsets.restype = C.c_int
    L.tsqa_frame_offsets.argtypes = [vp, C.c_uint32, vp, u64p]
    L.tsqa_walk_frames.restype = C.c_int
    L.tsqa_walk_frames.argtypes = [vp, C.c_size_t, C.c_uint32, vp, vp, vp, vp, u32p, u64p]
    L.tsqa_sharded_place_async.restype = C.c_int
    L.tsqa_sharded_place_async.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t, u64p, vp]
    L.tsqa_sharded_fetch_decode_async.restype = C.c_int
    L.tsqa_sharded_fetch_decode_async.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, C.c_size_t, vp, u64p, vp]
    L.tsqa_sharded_decode_again_async.restype = C.c_int
    L.tsqa_sharded_decode_again_async.argtypes = [vp, vp, vp, vp, vp]
    L.tsqa_encode_lookahead_state.restype = C.c_int
    L.tsqa_encode_lookahead_state.argtypes = []
    L.tsqa_copy_probe_shape.restype = C.c_char_p
    L.tsqa_copy_probe_shape.argtypes = [vp]
    L.tsqa_measure_copy.restype = C.c_int
    L.tsqa_measure_copy.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.tsqa_index_create.restype = C.c_int
    L.tsqa_index_create.argtypes = [vp, vp, C.c_size_t, C.POINTER(vp)]
    L.tsqa_index_destroy.restype = None
    L.tsqa_index_destroy.argtypes = [vp]
    L.tsqa_index_blocks.restype = C.c_uint32
    L.tsqa_index_blocks.argtypes = [vp]
    L.tsqa_index_total.restype = C.c_uint64
    L.tsqa_index_total.argtypes = [vp]
    L.tsqa_plan_ranges.restype = C.c_int
    L.tsqa_plan_ranges.argtypes = [vp, C.c_uint32, vp, C.c_uint32, C.c_size_t, vp, C.c_uint32, u32p]
    L.tsqa_decompress_ranges_async.restype = C.c_int
    L.tsqa_decompress_ranges_async.argtypes = [vp, vp, vp, C.c_uint32, vp, C.c_size_t, vp, vp]
    L.tsqa_decompress_ranges.restype = C.c_int
    L.tsqa_decompress_ranges.argtypes = [vp, vp, vp, C.c_uint32, vp, C.c_size_t, vp]
    L.tsqa_plan_batch.restype = C.c_int
    L.tsqa_plan_batch.argtypes = [vp, C.c_uint32, C.c_size_t, C.c_size_t, vp, vp]
    L.tsqa_compress_batch_async.restype = C.c_int
    L.tsqa_compress_batch_async.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp, vp]
    L.tsqa_compress_batch.restype = C.c_int
    L.tsqa_compress_batch.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp]
    L.tsqa_decompress_batch_async.restype = C.c_int
    L.tsqa_decompress_batch_async.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, vp, C.c_size_t, vp, vp, vp]
    L.tsqa_decompress_batch.restype = C.c_int
    L.tsqa_decompress_batch.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, vp, C.c_size_t, vp, vp, vp]
    L.tsqa_batch_bound.restype = C.c_size_t
    L.tsqa_batch_bound.argtypes = [C.c_size_t]
    L.tsqa_plan_packed.restype = C.c_int
    L.tsqa_plan_packed.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.tsqa_compress_batch_packed_async.restype = C.c_int
    L.tsqa_compress_batch_packed_async.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp]
    L.tsqa_compress_batch_packed.restype = C.c_int
    L.tsqa_compress_batch_packed.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp, vp]
    L.tsqa_decompress_batch_packed_async.restype = C.c_int
    L.tsqa_decompress_batch_packed_async.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp, C.c_uint32, vp, C.c_size_t, vp, vp, vp]
    L.tsqa_decompress_batch_items_async.restype = C.c_int
    L.tsqa_decompress_batch_items_async.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp]
    L.tsqa_plan_dense.restype = C.c_int
    L.tsqa_plan_dense.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, vp, vp, vp]
    L.tsqa_decompress_batch_packed_dense_async.restype = C.c_int
    L.tsqa_decompress_batch_packed_dense_async.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t,
                                                           vp, vp, vp, vp, vp, vp]
    L.tsqa_decompress_batch_packed_items_async.restype = C.c_int
    L.tsqa_plan_compress_tables.restype = C.c_int
    L.tsqa_plan_compress_tables.argtypes = [vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.tsqa_compress_batch_packed_tables_async.restype = C.c_int
    L.tsqa_compress_batch_packed_tables_async.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp,
                                                          C.c_size_t, vp, vp, vp, vp, vp, vp, vp]
    L.tsqa_decompress_batch_packed_items_async.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp]
    L.tsqa_plan_join.restype = C.c_int
    L.tsqa_plan_join.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, u32p, u64p, u64p]
    L.tsqa_join_async.restype = C.c_int
    L.tsqa_join_async.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
    L.tsqa_join.restype = C.c_int
    L.tsqa_join.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, szp, u32p, vp, vp, vp, vp]
    L.tsqa_profile_read_cut.restype = C.c_int
    L.tsqa_profile_read_cut.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.tsqa_plan_cut.restype = C.c_int
    L.tsqa_plan_cut.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, vp, u32p]
    L.tsqa_cut_async.restype = C.c_int
    L.tsqa_cut_async.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
    L.tsqa_cut.restype = C.c_int
    L.tsqa_cut.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.tsqa_plan_cut_items.restype = C.c_int
    L.tsqa_plan_cut_items.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, vp, u32p]
    L.tsqa_cut_items_async.restype = C.c_int
    L.tsqa_cut_items_async.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
    L.tsqa_cut_items.restype = C.c_int
    L.tsqa_cut_items.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.tsqa_profile_read_gather.restype = C.c_int
    L.tsqa_profile_read_gather.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.tsqa_profile_read_rows.restype = C.c_int
    L.tsqa_profile_read_rows.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.tsqa_plan_gather.restype = C.c_int
    L.tsqa_plan_gather.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, vp, vp, u64p, u32p]
    L.tsqa_gather_async.restype = C.c_int
    L.tsqa_gather_async.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.tsqa_gather.restype = C.c_int
    L.tsqa_gather.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.tsqa_plan_gather_rows.restype = C.c_int
    L.tsqa_plan_gather_rows.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, vp, vp, vp, u32p]
    for f in (L.tsqa_gather_rows_async, L.tsqa_gather_rows):
        f.restype = C.c_int
        f.argtypes = [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.tsqa_plan_records.restype = C.c_int
    L.tsqa_plan_records.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, vp, vp]
    for f in (L.tsqa_records_async, L.tsqa_records):
        f.restype = C.c_int
        f.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, vp, vp, vp, vp]
    L.tsqa_profile_read_records.restype = C.c_int
    L.tsqa_profile_read_records.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.tsqa_plan_find.restype = C.c_int
    L.tsqa_plan_find.argtypes = [vp, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, vp]
    for f in (L.tsqa_find_async, L.tsqa_find):
        f.restype = C.c_int
        f.argtypes = [vp, vp, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, vp, vp, vp]
    L.tsqa_profile_read_find.restype = C.c_int
    L.tsqa_profile_read_find.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.tsqa_plan_crc32.restype = C.c_int
    L.tsqa_plan_crc32.argtypes = [vp, vp, vp, C.c_uint32, vp, vp]
    for f in (L.tsqa_crc32_async, L.tsqa_crc32):
        f.restype = C.c_int
        f.argtypes = [vp, vp, C.c_uint32, vp, vp, vp, vp, vp, vp]
    L.tsqa_crc32_host.restype = C.c_uint32
    L.tsqa_crc32_host.argtypes = [C.c_uint32, vp, C.c_size_t]
    L.tsqa_crc32_combine.restype = C.c_uint32
    L.tsqa_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
    L.tsqa_profile_read_crc.restype = C.c_int
    L.tsqa_profile_read_crc.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.tsqa_plan_split.restype = C.c_int
    L.tsqa_plan_split.argtypes = [C.c_size_t, C.c_uint32, u32p, szp]
    L.tsqa_compress_device_split_async.restype = C.c_int
    L.tsqa_compress_device_split_async.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, C.c_size_t, vp, vp, vp, C.c_uint32, vp]
    L.tsqa_compress_device_split.restype = C.c_int
    L.tsqa_compress_device_split.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, C.c_size_t, szp, vp, C.c_uint32, vp]
    L.tsqa_plan_batch_split.restype = C.c_int
    L.tsqa_plan_batch_split.argtypes = [vp, C.c_uint32, C.c_size_t, C.c_uint32, C.c_uint32, vp, u64p]
    L.tsqa_compress_batch_packed_split_async.restype = C.c_int
    L.tsqa_compress_batch_packed_split_async.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t,
                                                         vp, vp, vp, vp, vp]
    L.tsqa_compress_batch_packed_split.restype = C.c_int
    L.tsqa_compress_batch_packed_split.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t,
                                                   vp, vp, vp, vp]
    L.tsqa_plan_compress_tables_split.restype = C.c_int
    L.tsqa_plan_compress_tables_split.argtypes = [vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.tsqa_compress_batch_packed_tables_split_async.restype = C.c_int
    L.tsqa_compress_batch_packed_tables_split_async.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                                C.c_uint32, vp, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tsqa_decompress_device_sized_async.restype = C.c_int
    L.tsqa_decompress_device_sized_async.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, vp, C.c_size_t, vp, vp, vp]
    L.tsqa_decompress_device_sized.restype = C.c_int
    L.tsqa_decompress_device_sized.argtypes = [vp, vp, C.c_size_t, C.c_uint32, vp, vp, C.c_size_t, szp, vp]
    L.tsqa_index_create_sized_async.restype = C.c_int
    L.tsqa_index_create_sized_async.argtypes = [vp, vp, C.c_size_t, C.c_uint64, C.c_uint32, vp, C.POINTER(vp), vp]
    L.tsqa_index_create_sized.restype = C.c_int
    L.tsqa_index_create_sized.argtypes = [vp, vp, C.c_size_t, C.c_uint64, C.c_uint32, vp, C.POINTER(vp), vp]
    L.tsqa_index_d_status.restype = vp
    L.tsqa_index_d_status.argtypes = [vp]
    L.tsqa_index_create_batch.restype = C.c_int
    L.tsqa_index_create_batch.argtypes = [vp, vp, C.c_size_t, vp, C.c_uint32, C.POINTER(vp), vp]
    L.tsqa_index_items.restype = C.c_uint32
    L.tsqa_index_items.argtypes = [vp]
    L.tsqa_index_item_total.restype = C.c_uint64
    L.tsqa_index_item_total.argtypes = [vp, C.c_uint32]
    L.tsqa_index_item_status.restype = C.c_int
    L.tsqa_index_item_status.argtypes = [vp, C.c_uint32]
    L.tsqa_plan_item_ranges.restype = C.c_int
    L.tsqa_plan_item_ranges.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, C.c_size_t, vp, C.c_uint32, u32p, vp, C.c_uint32, u32p]
    L.tsqa_decompress_item_ranges_async.restype = C.c_int
    L.tsqa_decompress_item_ranges_async.argtypes = [vp, vp, vp, C.c_uint32, vp, C.c_size_t, vp, vp]
    L.tsqa_decompress_item_ranges.restype = C.c_int
    L.tsqa_decompress_item_ranges.argtypes = [vp, vp, vp, C.c_uint32, vp, C.c_size_t, vp]
    L.tsqa_plan_index_packed.restype = C.c_int
    L.tsqa_plan_index_packed.argtypes = [vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp]
    L.tsqa_index_create_packed_async.restype = C.c_int
    L.tsqa_index_create_packed_async.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, C.POINTER(vp),
                                                 vp, vp, vp]
    L.tsqa_index_create_packed.restype = C.c_int
    L.tsqa_index_create_packed.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, C.POINTER(vp), vp, vp]
    L.tsqa_index_fetch.restype = C.c_int
    L.tsqa_index_fetch.argtypes = [vp, vp, vp]
    L.tsqa_index_device_tables.restype = C.c_int
    L.tsqa_index_device_tables.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.tsqCompress.restype = None
    L.tsqCompress.argtypes = [vp, vp, C.c_bool, C.c_uint32]
    L.tsqDecompress.restype = None
    L.tsqDecompress.argtypes = [vp, vp]
    _libs[ab] = L
    return L


class Range(C.Structure):
    """tsqa_range: uncompressed bytes [offset, offset + length) -> d_out + out_at"""
    _fields_ = [("offset", C.c_uint64), ("length", C.c_uint64), ("out_at", C.c_uint64)]


class RangeItem(C.Structure):
    """tsqa_range_item: bytes [lo, hi) of block `block` -> d_out + out_at"""
    _fields_ = [("block", C.c_uint32), ("lo", C.c_uint32), ("hi", C.c_uint32), ("pad", C.c_uint32), ("out_at", C.c_uint64)]


def _range_array(ranges):
    """(offset, length, out_at) triples -> a ctypes tsqa_range array"""
    arr = (Range * max(len(ranges), 1))()
    for k, (off, ln, at) in enumerate(ranges):
        arr[k] = Range(int(off), int(ln), int(at))
    return arr


def plan_ranges(out_start, ranges, out_cap: int, cap_items=None):
    """tsqa_plan_ranges (host only): out_start = the blocks' output starts, then the total; ranges = (offset, length, out_at)
    triples.  -> list of (block, lo, hi, out_at).  Raises TsqError(3) when the call is refused."""
    import numpy as np
    starts = np.ascontiguousarray(out_start, dtype=np.uint64)
    rr = _range_array(ranges)
    n = C.c_uint32(0)
    if cap_items is None:
        rc = lib().tsqa_plan_ranges(starts.ctypes.data, starts.size - 1, rr, len(ranges), out_cap, None, 0, C.byref(n))
        if rc and n.value == 0:
            raise TsqError(rc, "tsqa_plan_ranges refused the ranges")
        cap_items = n.value
    items = (RangeItem * max(cap_items, 1))()
    rc = lib().tsqa_plan_ranges(starts.ctypes.data, starts.size - 1, rr, len(ranges), out_cap, items, cap_items, C.byref(n))
    if rc:
        raise TsqError(rc, "tsqa_plan_ranges refused the ranges")
    return [(items[k].block, items[k].lo, items[k].hi, items[k].out_at) for k in range(n.value)]


def _cut_packed(codec, who: str, n: int, out, enqueue):
    """What RangeIndex.cut and BatchIndex.cut_items share: enqueue(room, d_offsets, d_sizes, d_totals, d_status) is the async call
    for n ranges, room None to measure.  Without `out` it measures first and makes the arena.  -> (the PackedBatch, d_offsets,
    d_sizes); a nonzero status raises TsqError with .item_status and .needed."""
    torch = codec.torch
    if out is not None and (out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.device != codec.device):
        raise TsqError(3, "out must be a contiguous uint8 tensor on the codec's device")
    i64 = lambda k: torch.empty(k, dtype=torch.int64, device=codec.device)
    d_offsets, d_sizes, d_totals, d_status = i64(n + 1), i64(n), i64(n), torch.empty(n, dtype=torch.int32, device=codec.device)

    def call(room):
        codec._join()
        enqueue(room, d_offsets, d_sizes, d_totals, d_status)
        codec._join()
        status, item_status = codec.status(), d_status.cpu().tolist()
        needed = int(d_offsets[n].item())
        refused = [st for st in item_status if st not in (0, 6)]
        if status and (room is not None or refused):         # (measuring: every accepted range reads 6)
            e = TsqError(max(refused) if refused else status, f"{who}: item statuses {item_status[:64]}{' ...' if n > 64 else ''}")
            e.item_status, e.needed = item_status, needed
            raise e
        return needed

    if out is None:
        out = torch.empty(max(call(None), 16), dtype=torch.uint8, device=codec.device)
    used = call(out)
    host = torch.cat([d_offsets, d_sizes, d_totals]).cpu().tolist()
    return PackedBatch(codec, out[:used], host[:n + 1], host[n + 1:2 * n + 1], host[2 * n + 1:]), d_offsets, d_sizes


class RangeIndex:
    """The frame table of a device-resident .tsq container (tsqa_index_create), for reads of byte ranges of its uncompressed data.
    Holds a reference to the container tensor, which must not change while the index is used."""

    def __init__(self, codec: "DeviceCodec", blob):
        self.codec, self.blob, self.L = codec, blob, codec.L
        self.h = C.c_void_p()
        # the index is made on the context's own stream: whatever the current stream still writes to the container comes first
        codec.torch.cuda.current_stream(codec.device).synchronize()
        rc = self.L.tsqa_index_create(codec.h, blob.data_ptr(), blob.numel(), C.byref(self.h))
        if rc:
            raise codec._err(rc)
        self.n_blocks = int(self.L.tsqa_index_blocks(self.h))
        self.total = int(self.L.tsqa_index_total(self.h))

    def close(self):
        if self.h:
            self.L.tsqa_index_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _out(self, out, n):
        if out is None:
            return self.codec.torch.empty(max(n, 1), dtype=self.codec.torch.uint8, device=self.codec.device)
        if out.dtype != self.codec.torch.uint8 or not out.is_cuda or not out.is_contiguous():
            raise TsqError(3, "out must be a contiguous uint8 CUDA tensor")
        return out

    def read_into(self, ranges, out, sync: bool = True) -> None:
        """The raw call: ranges = (offset, length, out_at) triples, bytes land at out[out_at:].  sync=False: on the current stream,
        nothing waited for, the status in codec.status()."""
        rr = _range_array(ranges)
        if sync:
            rc = self.L.tsqa_decompress_ranges(self.codec.h, self.h, rr, len(ranges), out.data_ptr(), out.numel(), self.codec._stream())
        else:
            rc = self.L.tsqa_decompress_ranges_async(self.codec.h, self.h, rr, len(ranges), out.data_ptr(), out.numel(),
                                                     self.codec._status.data_ptr(), self.codec._stream())
        if rc:
            raise self.codec._err(rc)

    def read(self, offset: int, length: int, out=None):
        """Bytes [offset, offset + length) of the uncompressed data -> a uint8 CUDA tensor (out[:length] when out is given)."""
        out = self._out(out, length)
        self.read_into([(offset, length, 0)], out)
        return out[:length]

    def _packed(self, ranges, out):
        at, triples = 0, []
        for off, ln in ranges:
            triples.append((off, ln, at))
            at += int(ln)
        out = self._out(out, at)
        return triples, out, [out[a:a + int(ln)] for (_, ln, a) in triples]

    def read_many(self, ranges, out=None):
        """One call for many (offset, length) ranges, packed back to back.  -> (packed tensor, per-range views into it)."""
        triples, out, views = self._packed(ranges, out)
        self.read_into(triples, out)
        return out[:sum(int(ln) for _, ln in ranges)], views

    def read_many_async(self, ranges, out=None):
        """read_many on the current torch stream, nothing waited for (like DeviceCodec.decompress_async): the status lands in
        codec.status()."""
        triples, out, views = self._packed(ranges, out)
        self.read_into(triples, out, sync=False)
        return out[:sum(int(ln) for _, ln in ranges)], views

    def cut(self, ranges, align: int = 16, out=None) -> "PackedBatch":
        """The block ranges `ranges` -- a list of (first, count), or a pair of int64 CUDA tensors (d_first, d_count) -- each as a
        .tsq container of its own, packed in one arena at multiples of `align` (DeviceCodec.cut_async: the frames are copied, nothing
        is decoded).  Without `out` the cut is measured first and an arena of exactly the bytes needed is made.  -> a PackedBatch
        whose lengths are the ranges' uncompressed sizes: decompress(), index() and join() take it.  A nonzero status raises
        TsqError with the item statuses in the text and in .item_status; for an `out` that is too small (6) .needed = the bytes a
        retry needs."""
        codec, torch = self.codec, self.codec.torch
        if isinstance(ranges, (tuple, list)) and len(ranges) == 2 and all(hasattr(t, "data_ptr") for t in ranges):
            d_first, d_count = ranges
        else:
            import numpy as np
            table = np.array([[int(f) for f, _ in ranges], [int(n) for _, n in ranges]], dtype=np.uint64).view(np.int64)
            d_first, d_count = torch.from_numpy(table).to(codec.device)
        n = int(d_first.numel())
        return _cut_packed(codec, "cut", n, out, lambda room, *tables: codec.cut_async(self, d_first, d_count, n, align, room, *tables))[0]

    def _gather(self, d_items, d_offsets, d_lengths, align, out, cap_pieces, range_status):
        codec, torch = self.codec, self.codec.torch
        n = int(d_offsets.numel())
        for name, t, dtypes in (("d_offsets", d_offsets, (torch.int64,)), ("d_lengths", d_lengths, (torch.int64,)),
                                ("d_items", d_items, (torch.int32, getattr(torch, "uint32", torch.int32)))):
            if t is not None and (t.dtype not in dtypes or t.device != codec.device or not t.is_contiguous() or t.numel() != n):
                raise TsqError(3, f"{name} must be a contiguous {str(dtypes[0])[6:]} tensor of {n} entries on the codec's device")
        if out is not None and (out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.device != codec.device):
            raise TsqError(3, "out must be a contiguous uint8 tensor on the codec's device")
        d_out_offsets = torch.empty(n + 1, dtype=torch.int64, device=codec.device)
        d_status = torch.empty(max(n, 1), dtype=torch.int32, device=codec.device)
        d_need = torch.empty(1, dtype=torch.int64, device=codec.device)
        if n == 0:                                           # (an empty tensor has no address to give: the call reads no table entry)
            d_offsets = d_lengths = d_need
            d_items = None
        if out is None or cap_pieces is None:
            # the two sums, measured: a call with no room refuses every range with bytes and still makes the whole layout
            codec._join()
            codec.gather_async(self, d_items, d_offsets, d_lengths, n, align, 1, torch.empty(1, dtype=torch.uint8, device=codec.device),
                               d_out_offsets, d_status, d_need, out_cap=0)
            codec._join()
            room, need = (int(x) for x in torch.stack([d_out_offsets[n], d_need[0]]).cpu().tolist())
            if out is None:
                out = torch.empty(max(room, 1), dtype=torch.uint8, device=codec.device)[:room]
            if cap_pieces is None:
                cap_pieces = max(min(need, 0xFFFFFFFF), 1)
        codec._join()
        codec.gather_async(self, d_items, d_offsets, d_lengths, n, align, cap_pieces, out if out.numel() else torch.empty(1, dtype=torch.uint8, device=codec.device),
                           d_out_offsets, d_status, d_need, out_cap=out.numel())
        codec._join()
        return (out, d_out_offsets, d_status[:n]) if range_status else (out, d_out_offsets)

    def gather(self, d_offsets, d_lengths, align: int = 1, out=None, cap_pieces=None, range_status: bool = False):
        """Bytes [d_offsets[k], d_offsets[k] + d_lengths[k]) of the uncompressed data for int64 CUDA tensors of offsets and lengths,
        planned on the device (DeviceCodec.gather_async): nothing about the ranges is read on the host.  -> (out, d_out_offsets):
        range k lies at out[d_out_offsets[k]:][:d_lengths[k]], d_out_offsets[n] is the room the ranges need; with range_status=True
        also the int32 verdict per range (0; 3 refused; 6 does not fit out or cap_pieces).  The largest verdict lands in
        codec.status().  On a stream of the caller's (torch.cuda.stream) the call is enqueued there and, with both `out` and
        `cap_pieces` given, nothing is waited for.  On torch's default stream the library runs on the context's own stream, which
        torch's work does not order itself against: there the wrapper waits for the device before and after the call.  Without
        `out` or `cap_pieces` the call is first run with no room, and the host WAITS ONCE for its two sums -- the bytes and the
        pieces needed -- because no bound on them is known to the host while the lengths are the device's."""
        return self._gather(None, d_offsets, d_lengths, align, out, cap_pieces, range_status)

    def _gather_rows(self, d_items, d_offsets, d_lengths, row_stride, pad, truncate, out, cap_pieces, row_status):
        codec, torch = self.codec, self.codec.torch
        first = next((t for t in (d_items, d_offsets, d_lengths) if t is not None), None)
        if first is None:
            raise TsqError(3, "gather_rows needs one of d_items, d_offsets and d_lengths: it says how many rows there are")
        n, row_stride = int(first.numel()), int(row_stride)
        for name, t, dtypes in (("d_offsets", d_offsets, (torch.int64,)), ("d_lengths", d_lengths, (torch.int64,)),
                                ("d_items", d_items, (torch.int32, getattr(torch, "uint32", torch.int32)))):
            if t is not None and (t.dtype not in dtypes or t.device != codec.device or not t.is_contiguous() or t.numel() != n):
                raise TsqError(3, f"{name} must be a contiguous {str(dtypes[0])[6:]} tensor of {n} entries on the codec's device")
        if out is not None and (out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.device != codec.device):
            raise TsqError(3, "out must be a contiguous uint8 tensor on the codec's device")
        if row_stride < 1 or (out is not None and out.numel() < n * row_stride):
            raise TsqError(3, f"gather_rows: {n} rows of {row_stride} B do not fit out")
        flags = ROWS_TRUNCATE if truncate else 0
        d_row_lengths = torch.empty(max(n, 1), dtype=torch.int64, device=codec.device)
        d_status = torch.empty(max(n, 1), dtype=torch.int32, device=codec.device)
        d_need = torch.empty(2, dtype=torch.int64, device=codec.device)
        if n == 0:                                           # (an empty tensor has no address to give: the call reads no table entry)
            d_items = d_offsets = d_lengths = None
        if cap_pieces is None:
            # the piece sum, measured: a call without an output makes every table and decodes nothing
            codec._join()
            codec.gather_rows_async(self, d_items, d_offsets, d_lengths, n, row_stride, flags, pad, 1, None, d_row_lengths, d_status, d_need)
            codec._join()
            cap_pieces = max(min(int(d_need[0].item()), 0xFFFFFFFF), 1)
        if out is None:
            out = torch.empty(max(n * row_stride, 1), dtype=torch.uint8, device=codec.device)
        codec._join()
        codec.gather_rows_async(self, d_items, d_offsets, d_lengths, n, row_stride, flags, pad, cap_pieces, out, d_row_lengths, d_status, d_need)
        codec._join()
        rows = out[:n * row_stride].view(n, row_stride)
        return (rows, d_row_lengths[:n], d_status[:n]) if row_status else (rows, d_row_lengths[:n])

    def gather_rows(self, d_offsets, d_lengths, row_stride: int, pad: int = 0, truncate: bool = False, out=None, cap_pieces=None,
                    row_status: bool = False):
        """gather() into fixed-stride padded rows (DeviceCodec.gather_rows_async): bytes [d_offsets[k], d_offsets[k] + d_lengths[k])
        land in row k of a [n, row_stride] uint8 tensor -- a view of `out` --, the rest of every row is `pad` (0..255; -1 leaves
        it as it was), and lengths[k] (an int64 CUDA tensor) is what row k got.  -> (rows, lengths), with row_status=True also the
        int32 verdict per row: 0; 3 refused; 6 longer than row_stride (that row alone; truncate=True delivers its first row_stride
        bytes instead) or past cap_pieces.  A row with a nonzero verdict is all pad and has length 0.  d_offsets None: every offset
        is 0; d_lengths None: to the end of the data.  With `out` and `cap_pieces` given, on a stream of the caller's, nothing is
        waited for; without cap_pieces the call is measured first and the host WAITS ONCE for the piece sum."""
        return self._gather_rows(None, d_offsets, d_lengths, row_stride, pad, truncate, out, cap_pieces, row_status)

    def records(self, delim: int = 10, keep_delim: bool = False, flat: bool = False, cap_records=None, sync: bool = True) -> "RecordTable":
        """Where the records of the data are, for a delimiter byte (DeviceCodec.records_async): a record starts at byte 0 of every
        item and behind every delimiter but one at the item's last byte, and ends in front of the next delimiter or at the item's
        end.  The data is decoded and compared on the device; no decoded copy is made -- the scratch is a bit per byte.  keep_delim:
        a record's length includes its terminator; flat: offsets count from the start of the whole data (what gather() without
        items takes), else from the record's own item.  -> a RecordTable whose tensors gather() and gather_rows() take.
        cap_records None: the call is run twice -- once with no tables, which only measures, then, after ONE host read of the
        count, with tables of exactly that many entries: two calls, one host read, two decodes.  cap_records given: ONE enqueue on
        the current stream with no host read; the tables have cap_records entries, the records below it are written, and
        table.status reads 6 when there are more (table.need[0] says how many).  sync=False with cap_records: nothing is waited
        for.  Otherwise the call is waited for and a refused index (4) or a malformed stream (5) raises TsqError."""
        codec, torch = self.codec, self.codec.torch
        # (a DeviceBatchIndex before fetch() is refused by the library, with the text that names tsqa_index_fetch)
        flags = (RECORDS_KEEP_DELIM if keep_delim else 0) | (RECORDS_FLAT if flat else 0)
        n_items = int(self.L.tsqa_index_items(self.h))
        i64 = lambda k: torch.empty(max(int(k), 1), dtype=torch.int64, device=codec.device)
        item_first, need = i64(n_items + 1)[:n_items + 1], i64(2)
        status = torch.empty(1, dtype=torch.int32, device=codec.device)
        measured = cap_records is None
        if measured:
            codec._join()
            codec.records_async(self, delim, flags, 0, None, None, None, item_first, need, status)
            codec._join()
            cap_records = int(need[0].item())
        cap_records = int(cap_records)
        offsets, lengths = i64(cap_records)[:cap_records], i64(cap_records)[:cap_records]
        items = torch.empty(max(cap_records, 1), dtype=torch.int32, device=codec.device)[:cap_records]
        codec._join()
        codec.records_async(self, delim, flags, cap_records, items if cap_records else None, offsets if cap_records else None,
                            lengths if cap_records else None, item_first, need, status)
        codec._join()
        table = RecordTable(self, offsets, lengths, items, item_first, need, status, flat)
        if sync or measured:
            st = int(status.item())
            if st not in (0, 6):
                raise TsqError(st, "records: the device reported a refused index (4) or a malformed stream (5)")
        return table

    def find(self, needle: bytes, flat: bool = False, cap_hits=None, sync: bool = True) -> "HitTable":
        """Where the byte string `needle` (1 .. FIND_MAX_NEEDLE bytes) occurs in the data (DeviceCodec.find_async): every p with
        data[p : p + len(needle)] == needle inside one item, overlapping occurrences included.  The data is decoded and compared on
        the device; no decoded copy is made -- the scratch is a bit per byte and 32 bytes per block.  flat: offsets count from the
        start of the whole data, else from the hit's own item.  -> a HitTable.  cap_hits None: the call is run twice -- once with
        no tables, which only measures, then, after ONE host read of the count, with tables of exactly that many entries.
        cap_hits given: ONE enqueue on the current stream with no host read; the hits below it are written, and table.status
        reads 6 when there are more (table.need[0] says how many).  sync=False with cap_hits: nothing is waited for.  Otherwise
        the call is waited for and a refused index (4) or a malformed stream (5) raises TsqError."""
        codec, torch = self.codec, self.codec.torch
        needle = bytes(needle)
        flags = FIND_FLAT if flat else 0
        n_items = int(self.L.tsqa_index_items(self.h))
        i64 = lambda k: torch.empty(max(int(k), 1), dtype=torch.int64, device=codec.device)
        item_first, need = i64(n_items + 1)[:n_items + 1], i64(1)
        status = torch.empty(1, dtype=torch.int32, device=codec.device)
        measured = cap_hits is None
        if measured:
            codec._join()
            codec.find_async(self, needle, flags, 0, None, None, item_first, need, status)
            codec._join()
            cap_hits = int(need[0].item())
        cap_hits = int(cap_hits)
        offsets = i64(cap_hits)[:cap_hits]
        items = torch.empty(max(cap_hits, 1), dtype=torch.int32, device=codec.device)[:cap_hits]
        codec._join()
        codec.find_async(self, needle, flags, cap_hits, items if cap_hits else None, offsets if cap_hits else None, item_first, need, status)
        codec._join()
        table = HitTable(self, offsets, items, item_first, need, status, flat, len(needle))
        if sync or measured:
            st = int(status.item())
            if st not in (0, 6):
                raise TsqError(st, "find: the device reported a refused index (4) or a malformed stream (5)")
        return table

    def crc32(self, blocks: bool = False, all: bool = True, sync: bool = True) -> "CrcTable":
        """zlib's CRC-32 of every item's data (DeviceCodec.crc32_async): the value zlib.crc32 gives for the bytes a decompress would
        write.  The data is decoded and checksummed on the device; no decoded copy is made -- the scratch is 4 bytes per block.  all:
        the CRC of the whole data too; blocks: one CRC per block too (they fold into the items' with crc32_combine).  -> a CrcTable.
        One enqueue on the current stream with no host read; sync=True then waits and raises TsqError for a refused index (4), and
        for a malformed stream (5) unless it cost only some of several items -- then the table's status says which."""
        codec = self.codec
        codec._join()
        table = codec.crc32_async(self, blocks=blocks, all=all)
        codec._join()
        if sync:
            table.check()
        return table


class CrcTable:
    """What RangeIndex.crc32 gives: items (one CRC per item), all (the whole data's CRC, one entry, or None) and blocks (one per block,
    or None) -- the uint32 values as int64 CUDA tensors, made on demand from d_items, d_all and d_blocks, the int32 tensors the
    device wrote --; status (int32 per item: 0, the index's own status for an item it refused, 5 for an item with a malformed
    stream; the CRC of both is 0) and d_status (int32, 1: 0, 4 a refused sized index, 5 when any item was raised to it).  All are
    valid behind the stream the call was enqueued on."""

    def __init__(self, index, d_items, status, d_blocks, d_all, d_status):
        self.index, self.d_items, self.status, self.d_blocks, self.d_all, self.d_status = index, d_items, status, d_blocks, d_all, d_status

    @property
    def items(self):
        return self.d_items.long() & 0xFFFFFFFF

    @property
    def blocks(self):
        return None if self.d_blocks is None else self.d_blocks.long() & 0xFFFFFFFF

    @property
    def all(self):
        return None if self.d_all is None else self.d_all.long() & 0xFFFFFFFF

    def check(self) -> "CrcTable":
        """Waits for the call.  Raises TsqError when the index was refused (4), or when a malformed stream (5) left no healthy
        item; -> the table otherwise (with status 5 on the items it cost)."""
        st = int(self.d_status.item())
        if st == 4 or (st != 0 and not bool((self.status == 0).any().item())):
            raise TsqError(st, "crc32: the device reported a refused index (4) or a malformed stream (5)")
        return self


class HitTable:
    """What RangeIndex.find gives: offsets (int64, each hit's first byte) and items (int32) of cap_hits entries, of which the first
    min(n, cap_hits) are hits; item_first (int64, items + 1: each item's first hit number, then the count); need (int64, 1: the count
    of all hits) and status (int32: 0, 6 when there are more hits than entries, 4, 5) -- all CUDA tensors, valid behind the stream the
    call was enqueued on.  needle_len is the needle's length; n reads `need` on the host (it waits)."""

    def __init__(self, index, offsets, items, item_first, need, status, flat: bool, needle_len: int):
        self.index, self.offsets, self.items, self.item_first, self.need, self.status, self.flat, self.needle_len = (
            index, offsets, items, item_first, need, status, flat, needle_len)
        self._n = None

    @property
    def n(self) -> int:
        if self._n is None:
            self._n = int(self.need[0].item())
        return self._n


class RecordTable:
    """What RangeIndex.records gives: offsets, lengths (int64) and items (int32) of cap_records entries, of which the first
    min(n, cap_records) are records; item_first (int64, items + 1: each item's first record number, then the count); need (int64:
    the count of all records, the largest record length) and status (int32: 0, 6 when there are more records than entries, 4, 5) --
    all CUDA tensors, valid behind the stream the call was enqueued on.  n and max_length read `need` on the host (they wait)."""

    def __init__(self, index, offsets, lengths, items, item_first, need, status, flat: bool):
        self.index, self.offsets, self.lengths, self.items, self.item_first, self.need, self.status, self.flat = (
            index, offsets, lengths, items, item_first, need, status, flat)
        self._need = None

    def _read_need(self):
        if self._need is None:
            self._need = [int(x) for x in self.need.cpu().tolist()]
        return self._need

    @property
    def n(self) -> int:
        return self._read_need()[0]

    @property
    def max_length(self) -> int:
        return self._read_need()[1]

    def gather_rows(self, sel, row_stride=None, pad: int = 0, truncate: bool = False, out=None, cap_pieces=None, row_status: bool = False):
        """The records numbered sel (an int64 CUDA tensor of record numbers below the table's entries) as rows: items[sel],
        offsets[sel], lengths[sel] go to the index's gather_rows (torch indexing; nothing new on the device).  row_stride None:
        max_length, which truncates nothing (one host read)."""
        if row_stride is None:
            row_stride = max(self.max_length, 1)
        d_items = None if self.flat else self.items[sel].contiguous()
        return self.index._gather_rows(d_items, self.offsets[sel].contiguous(), self.lengths[sel].contiguous(), row_stride, pad, truncate, out,
                                       cap_pieces, row_status)

    def containing(self, hits: "HitTable"):
        """The sorted unique numbers of the records that hold a whole hit of `hits`: offsets[r] <= hit and hit + needle_len <=
        offsets[r] + lengths[r] (torch only: a searchsorted of the hits in the records' flat offsets, which grow with the record
        number; nothing new on the device).  Both tables must have been made with flat=True; ValueError otherwise.  Entries at
        or past either table's count (room to spare behind cap_records or cap_hits) are left out on the device, from the need
        words, with no host read; what a table that overflowed (status 6) lacks is lacking here too."""
        if not (self.flat and hits.flat):
            raise ValueError("RecordTable.containing needs both tables made with flat=True")
        torch = self.index.codec.torch
        if self.offsets.numel() == 0 or hits.offsets.numel() == 0:
            return torch.empty(0, dtype=torch.int64, device=self.offsets.device)
        live = lambda t, need: torch.arange(t.numel(), device=t.device) < need[0]
        rec_live = live(self.offsets, self.need)
        starts = torch.where(rec_live, self.offsets, torch.full_like(self.offsets, (1 << 63) - 1))        # (sorted still)
        # the last record that starts at or before the hit is the only one that can hold it (starts are strictly increasing)
        r = torch.searchsorted(starts, hits.offsets, right=True) - 1
        ok = (r >= 0) & live(hits.offsets, hits.need)
        r = r.clamp(min=0)
        ok &= rec_live[r] & (hits.offsets + hits.needle_len <= self.offsets[r] + self.lengths[r])
        return torch.unique(r[ok])


RECORDS_KEEP_DELIM, RECORDS_FLAT = 1, 2          # TSQA_RECORDS_KEEP_DELIM, TSQA_RECORDS_FLAT
FIND_FLAT, FIND_MAX_NEEDLE = 2, 16               # TSQA_FIND_FLAT, TSQA_FIND_MAX_NEEDLE


def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """tsqa_crc32_combine (host only): zlib's crc32_combine -- the CRC-32 of A | B from crc32(A), crc32(B) and B's length in bytes."""
    return int(lib().tsqa_crc32_combine(int(crc_a) & 0xFFFFFFFF, int(crc_b) & 0xFFFFFFFF, int(len_b)))


def crc32_host(data, crc: int = 0) -> int:
    """tsqa_crc32_host (host only): zlib.crc32(data, crc) by the library's own tables."""
    import numpy as np
    buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
    return int(lib().tsqa_crc32_host(int(crc) & 0xFFFFFFFF, buf.ctypes.data if buf.size else None, buf.size))


def plan_crc32(data, item_at, item_status=None):
    """tsqa_plan_crc32 (host only): the rule of RangeIndex.crc32 applied to decoded bytes on the host.  data, item_at, item_status: as
    in plan_records.  -> (item_crc: uint32 numpy, 0 for an empty or refused item; the CRC of the whole data, refused items left
    out).  Raises TsqError(3) when the arguments are refused."""
    import numpy as np
    buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
    at = np.ascontiguousarray(np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in item_at], dtype=np.uint64))
    n_items = len(at) - 1
    if n_items >= 1 and int(at[-1]) > buf.size:
        raise TsqError(3, "tsqa_plan_crc32: the items end past the data")
    st = None if item_status is None else np.ascontiguousarray(np.array([int(x) for x in item_status], dtype=np.int32))
    if st is not None and len(st) != n_items:
        raise TsqError(3, "tsqa_plan_crc32 takes one status per item")
    crc, whole = np.zeros(max(n_items, 1), dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    rc = lib().tsqa_plan_crc32(buf.ctypes.data if buf.size else None, at.ctypes.data, None if st is None else st.ctypes.data, max(n_items, 0),
                               crc.ctypes.data, whole.ctypes.data)
    if rc:
        raise TsqError(rc, "tsqa_plan_crc32 refused the arguments")
    return crc[:n_items], int(whole[0])


def plan_find(data, item_at, needle, item_status=None, flat: bool = False, cap_hits=None):
    """tsqa_plan_find (host only): the rule of RangeIndex.find applied to decoded bytes on the host.  data, item_at, item_status: as
    in plan_records.  cap_hits None: counts first, then fills tables of that many entries.  -> (items, offsets: the hits below
    cap_hits; item_first_hit, n_items + 1; the count).  Raises TsqError(3) when the arguments are refused."""
    import numpy as np
    buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
    at = np.ascontiguousarray(np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in item_at], dtype=np.uint64))
    n_items = len(at) - 1
    if n_items >= 1 and int(at[-1]) > buf.size:
        raise TsqError(3, "tsqa_plan_find: the items end past the data")
    st = None if item_status is None else np.ascontiguousarray(np.array([int(x) for x in item_status], dtype=np.int32))
    if st is not None and len(st) != n_items:
        raise TsqError(3, "tsqa_plan_find takes one status per item")
    needle = bytes(needle)
    nd = np.frombuffer(needle + b"\0", dtype=np.uint8)       # (never empty: the length says how much of it counts)
    first, need = np.zeros(max(n_items, 0) + 1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    ptr = lambda t: None if t is None else t.ctypes.data

    def call(cap, items, offsets):
        rc = lib().tsqa_plan_find(buf.ctypes.data if buf.size else None, at.ctypes.data, ptr(st), max(n_items, 0), nd.ctypes.data, len(needle),
                                  FIND_FLAT if flat else 0, cap, ptr(items), ptr(offsets), first.ctypes.data, need.ctypes.data)
        if rc:
            raise TsqError(rc, "tsqa_plan_find refused the arguments")
    if cap_hits is None:
        call(0, None, None)
        cap_hits = int(need[0])
    cap = int(cap_hits)
    items, offsets = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint64)
    call(cap, items, offsets)
    k = min(cap, int(need[0]))
    return items[:k], offsets[:k], first, int(need[0])


def plan_records(data, item_at, item_status=None, delim: int = 10, keep_delim: bool = False, flat: bool = False, cap_records=None):
    """tsqa_plan_records (host only): the rule of RangeIndex.records applied to decoded bytes on the host.  data: the concatenation
    of the items' data (bytes or a uint8 array); item_at: the items' starts in it, n_items + 1; item_status: nonzero refuses an
    item.  cap_records None: counts first, then fills tables of that many entries.  -> (items, offsets, lengths: the records below
    cap_records; item_first_record, n_items + 1; [the count, the largest length]).  Raises TsqError(3) when the arguments are refused."""
    import numpy as np
    buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
    at = np.ascontiguousarray(np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in item_at], dtype=np.uint64))
    n_items = len(at) - 1
    if n_items >= 1 and int(at[-1]) > buf.size:
        raise TsqError(3, "tsqa_plan_records: the items end past the data")
    st = None if item_status is None else np.ascontiguousarray(np.array([int(x) for x in item_status], dtype=np.int32))
    if st is not None and len(st) != n_items:
        raise TsqError(3, "tsqa_plan_records takes one status per item")
    flags = (RECORDS_KEEP_DELIM if keep_delim else 0) | (RECORDS_FLAT if flat else 0)
    first, need = np.zeros(max(n_items, 0) + 1, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    ptr = lambda t: None if t is None else t.ctypes.data

    def call(cap, items, offsets, lengths):
        rc = lib().tsqa_plan_records(buf.ctypes.data if buf.size else None, at.ctypes.data, ptr(st), max(n_items, 0), int(delim), flags, cap,
                                     ptr(items), ptr(offsets), ptr(lengths), first.ctypes.data, need.ctypes.data)
        if rc:
            raise TsqError(rc, "tsqa_plan_records refused the arguments")
    if cap_records is None:
        call(0, None, None, None)
        cap_records = int(need[0])
    cap = int(cap_records)
    items, offsets, lengths = np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint64)
    call(cap, items, offsets, lengths)
    k = min(cap, int(need[0]))
    return items[:k], offsets[:k], lengths[:k], first, [int(x) for x in need]


class SizedIndex(RangeIndex):
    """The index of a container of short blocks, made on the device from its table of stream sizes (tsqa_index_create_sized*): the
    caller states the geometry (total bytes cut every block_len), the device places the frames and proves it.  sync=False: made on
    the current torch stream with nothing waited for, so compress_split_async -> index_sized -> read_many_async is one chain; a
    container that is refused then shows in status(), and in the status of every read.  Holds references to the container and the
    table, which must not change while the index is made or used."""

    def __init__(self, codec: "DeviceCodec", blob, total: int, block_len: int, block_sizes, sync: bool = True):
        self.codec, self.blob, self.table, self.L = codec, blob, block_sizes, codec.L
        self.h = C.c_void_p()
        codec._check_table(block_sizes, plan_split(total, block_len)[0], at_least=True)
        make = self.L.tsqa_index_create_sized if sync else self.L.tsqa_index_create_sized_async
        rc = make(codec.h, blob.data_ptr(), blob.numel(), int(total), int(block_len), block_sizes.data_ptr(), C.byref(self.h), codec._stream())
        if rc:
            raise codec._err(rc)
        self.n_blocks = int(self.L.tsqa_index_blocks(self.h))
        self.total = int(self.L.tsqa_index_total(self.h))
        self.block_len = int(block_len)

    def status(self) -> int:
        """The walk's verdict (tsqa_index_d_status), 0 or 4, as a read of nothing on the current stream reports it: waits for
        that stream."""
        if not self.h or not self.L.tsqa_index_d_status(self.h):
            raise TsqError(3, "the index is closed")
        one = self.codec.torch.empty(1, dtype=self.codec.torch.uint8, device=self.codec.device)
        return int(self.L.tsqa_decompress_ranges(self.codec.h, self.h, None, 0, one.data_ptr(), 1, self.codec._stream()))


class BatchItem(C.Structure):
    """tsqa_batch_item: input bytes [in_at, in_at + in_len) -> output range [out_at, out_at + out_cap)"""
    _fields_ = [("in_at", C.c_uint64), ("in_len", C.c_uint64), ("out_at", C.c_uint64), ("out_cap", C.c_uint64)]


def _batch_array(items):
    """(in_at, in_len, out_at, out_cap) quadruples -> a ctypes tsqa_batch_item array"""
    arr = (BatchItem * max(len(items), 1))()
    for k, (a, n, o, cap) in enumerate(items):
        arr[k] = BatchItem(int(a), int(n), int(o), int(cap))
    return arr


def plan_batch(items, in_size: int, out_size: int, n_blocks=None):
    """tsqa_plan_batch (host only): items = (in_at, in_len, out_at, out_cap); n_blocks None: a compress batch, else the stated block
    count per container.  -> each item's first block in the batch, then the batch's block count.  Raises TsqError(3) when refused."""
    import numpy as np
    first = np.zeros(len(items) + 1, dtype=np.uint64)
    nb = None if n_blocks is None else np.ascontiguousarray(n_blocks, dtype=np.uint32)
    rc = lib().tsqa_plan_batch(_batch_array(items), len(items), in_size, out_size, None if nb is None else nb.ctypes.data, first.ctypes.data)
    if rc:
        raise TsqError(rc, "tsqa_plan_batch refused the batch")
    return [int(x) for x in first]


def batch_bound(n: int) -> int:
    """Room that always holds the container of an n-byte item, much tighter than container_bound below a block: the header, then
    per block its frame word and a stream of at most every byte a literal of its own (n + n/8 + n/2 + 11), and never more than
    TSQ_OUTPUT_SZ."""
    cap, left = 16, n
    while left > 0:
        k = min(left, BLOCK_SZ)
        cap += 3 + min(OUTPUT_SZ, 11 + k + (k >> 3) + (k >> 1))
        left -= k
    return cap


def plan_split(n: int, block_len: int):
    """tsqa_plan_split (host only): an input of n bytes cut into blocks of block_len, a power of two from 2^12 to 2^22 -> (the block
    count, the room that always holds the container).  Raises TsqError(3) when refused."""
    nb, bound = C.c_uint32(0), C.c_size_t(0)
    if not 0 <= n < 1 << 64 or not 0 <= block_len < 1 << 32:
        raise TsqError(3, "tsqa_plan_split refused the arguments")
    rc = lib().tsqa_plan_split(n, block_len, C.byref(nb), C.byref(bound))
    if rc:
        raise TsqError(rc, "tsqa_plan_split refused the arguments")
    return int(nb.value), int(bound.value)


def plan_batch_split(items, in_size: int, block_len: int, align: int = 16):
    """tsqa_plan_batch_split (host only): items = (in_at, in_len, ...) cut every block_len bytes, a power of two from 2^12 to 2^22
    -> (each item's first block in the batch, then the batch's block count; the room that always holds the packed arena: the sum
    of round_up(plan_split's bound, align)).  Raises TsqError(3) when refused."""
    import numpy as np
    first = np.zeros(len(items) + 1, dtype=np.uint64)
    bound = C.c_uint64(0)
    if not 0 <= block_len < 1 << 32 or not 0 <= align < 1 << 32:
        raise TsqError(3, "tsqa_plan_batch_split refused the batch")
    quads = [(it[0], it[1], 0, 0) for it in items]
    rc = lib().tsqa_plan_batch_split(_batch_array(quads), len(quads), in_size, block_len, align, first.ctypes.data, C.byref(bound))
    if rc:
        raise TsqError(rc, "tsqa_plan_batch_split refused the batch")
    return [int(x) for x in first], int(bound.value)


def plan_packed(sizes, align: int = 16):
    """tsqa_plan_packed (host only): the packed layout of containers of the given sizes -> their offsets, then the bytes used
    (offsets[i + 1] = round_up(offsets[i] + sizes[i], align), the last without the rounding).  Raises TsqError(3) when refused."""
    import numpy as np
    sz = np.ascontiguousarray(sizes, dtype=np.uint64)
    offsets = np.zeros(len(sz) + 1, dtype=np.uint64)
    rc = lib().tsqa_plan_packed(sz.ctypes.data, len(sz), align, offsets.ctypes.data)
    if rc:
        raise TsqError(rc, "tsqa_plan_packed refused the sizes")
    return [int(x) for x in offsets]


def plan_dense(totals, blocks, align: int = 16, out_size: int = 0, cap_blocks: int = 0):
    """tsqa_plan_dense (host only): the dense output layout of items with these uncompressed sizes and block counts (blocks[i] == 0:
    an item refused at its header) -> (out_offsets, then the bytes needed; first_block, then the blocks needed; n_fit: the first
    accepted item that does not fit out_size bytes and cap_blocks blocks, len(totals) when all do)."""
    import numpy as np
    tot = np.ascontiguousarray(totals, dtype=np.uint64)
    nb = np.ascontiguousarray(blocks, dtype=np.uint32)
    offsets, first = np.zeros(len(tot) + 1, dtype=np.uint64), np.zeros(len(tot) + 1, dtype=np.uint64)
    n_fit = C.c_uint32(0)
    rc = lib().tsqa_plan_dense(tot.ctypes.data, nb.ctypes.data, len(tot), align, out_size, cap_blocks, offsets.ctypes.data, first.ctypes.data,
                               C.byref(n_fit))
    if rc:
        raise TsqError(rc, "tsqa_plan_dense refused the arguments")
    return [int(x) for x in offsets], [int(x) for x in first], int(n_fit.value)


def plan_compress_tables(in_offsets, in_sizes, in_size: int, align: int = 16, cap_blocks: int = 0):
    """tsqa_plan_compress_tables (host only): what DeviceCodec.compress_batch_packed_tables_async decides before it encodes, from
    host copies of its tables -> (first_block, then the blocks needed; item_status: 0, 3 for a place outside the input, 6 for an
    accepted item outside the prefix that fits cap_blocks; bound: the room that always holds the arena; n_fit)."""
    import numpy as np
    at = np.ascontiguousarray(in_offsets, dtype=np.uint64)
    sz = np.ascontiguousarray(in_sizes, dtype=np.uint64)
    first, status = np.zeros(len(sz) + 1, dtype=np.uint64), np.zeros(len(sz), dtype=np.int32)
    bound, n_fit = C.c_uint64(0), C.c_uint32(0)
    rc = lib().tsqa_plan_compress_tables(at.ctypes.data, sz.ctypes.data, min(len(at), len(sz)), in_size, align, cap_blocks, first.ctypes.data,
                                         status.ctypes.data, C.byref(bound), C.byref(n_fit))
    if rc:
        raise TsqError(rc, "tsqa_plan_compress_tables refused the arguments")
    return [int(x) for x in first], [int(x) for x in status], int(bound.value), int(n_fit.value)


def plan_compress_tables_split(in_offsets, in_sizes, in_size: int, block_len: int, align: int = 16, cap_blocks: int = 0):
    """tsqa_plan_compress_tables_split (host only): plan_compress_tables with the items cut every block_len bytes; an item of more
    than 2^32 - 1 blocks reads 3 as well, and the bound's term is plan_split's."""
    import numpy as np
    at = np.ascontiguousarray(in_offsets, dtype=np.uint64)
    sz = np.ascontiguousarray(in_sizes, dtype=np.uint64)
    first, status = np.zeros(len(sz) + 1, dtype=np.uint64), np.zeros(len(sz), dtype=np.int32)
    bound, n_fit = C.c_uint64(0), C.c_uint32(0)
    if not 0 <= block_len < 1 << 32:
        raise TsqError(3, "tsqa_plan_compress_tables_split refused the arguments")
    rc = lib().tsqa_plan_compress_tables_split(at.ctypes.data, sz.ctypes.data, min(len(at), len(sz)), in_size, block_len, align, cap_blocks,
                                               first.ctypes.data, status.ctypes.data, C.byref(bound), C.byref(n_fit))
    if rc:
        raise TsqError(rc, "tsqa_plan_compress_tables_split refused the arguments")
    return [int(x) for x in first], [int(x) for x in status], int(bound.value), int(n_fit.value)


def plan_join(frame_bytes, blocks, totals):
    """tsqa_plan_join (host only): the join of containers with these frame bytes (from a container's start to the end of its last
    frame), block counts and uncompressed sizes -> (body_at, then the joined size; first_block, then the block sum; the joined
    header's block count and total; the joined size).  Raises TsqError(3) when refused, and TsqError(6) -- with .body_at and
    .first_block, which are still made -- when the block sum does not fit 32 bits."""
    import numpy as np
    fb = np.ascontiguousarray(frame_bytes, dtype=np.uint64)
    nb = np.ascontiguousarray(blocks, dtype=np.uint32)
    tot = np.ascontiguousarray(totals, dtype=np.uint64)
    n = min(len(fb), len(nb), len(tot))
    body_at, first = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    n_blocks, total, size = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    rc = lib().tsqa_plan_join(fb.ctypes.data, nb.ctypes.data, tot.ctypes.data, n, body_at.ctypes.data, first.ctypes.data, C.byref(n_blocks),
                              C.byref(total), C.byref(size))
    if rc == 6:
        e = TsqError(rc, "the joined block count does not fit 32 bits")
        e.body_at, e.first_block = [int(x) for x in body_at], [int(x) for x in first]
        raise e
    if rc:
        raise TsqError(rc, "tsqa_plan_join refused the arguments")
    return [int(x) for x in body_at], [int(x) for x in first], int(n_blocks.value), int(total.value), int(size.value)


def plan_cut(frame_at, out_start, ranges, align: int = 16, out_size: int = 0):
    """tsqa_plan_cut (host only): the cut of the block ranges (first, count) out of a container with these n_blocks + 1 frame
    boundaries (tsqa_walk_frames' frame_at with the end of the last frame appended) and block starts (out_start, as plan_ranges takes
    it) -> (offsets, then the bytes needed; sizes; totals; item_status: 0, 3 for a range outside the container, 6 for an accepted
    range that does not fit out_size; n_fit).  Raises TsqError(3) when refused."""
    import numpy as np
    first = np.array([int(f) for f, _ in ranges], dtype=np.uint64)
    count = np.array([int(n) for _, n in ranges], dtype=np.uint64)
    return _plan_cut("tsqa_plan_cut", frame_at, out_start, (first, count), len(first), align, out_size)


def _plan_cut(name: str, frame_at, out_start, tables, n: int, align: int, out_size: int):
    """What plan_cut and plan_cut_items share: the planner `name` of the C ABI over n ranges.  tables: what it takes between n_blocks
    and n_ranges, numpy arrays (or None) passed by address and ints as they are."""
    import numpy as np
    fa = np.ascontiguousarray(frame_at, dtype=np.uint64)
    os_ = np.ascontiguousarray(out_start, dtype=np.uint64)
    if len(fa) != len(os_) or len(fa) < 1:
        raise TsqError(3, f"{name} takes n_blocks + 1 frame boundaries and as many block starts")
    offsets, sizes, totals = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
    status, n_fit = np.zeros(max(n, 1), dtype=np.int32), C.c_uint32(0)
    rc = getattr(lib(), name)(fa.ctypes.data, os_.ctypes.data, len(fa) - 1, *(a.ctypes.data if hasattr(a, "ctypes") else a for a in tables),
                              n, align, out_size, offsets.ctypes.data, sizes.ctypes.data, totals.ctypes.data, status.ctypes.data, C.byref(n_fit))
    if rc:
        raise TsqError(rc, f"{name} refused the arguments")
    return [int(x) for x in offsets], [int(x) for x in sizes[:n]], [int(x) for x in totals[:n]], [int(x) for x in status[:n]], int(n_fit.value)


def plan_cut_items(frame_at, out_start, item_first_block, items, ranges, align: int = 16, out_size: int = 0):
    """tsqa_plan_cut_items (host only): plan_cut through an index of several items.  frame_at: n_blocks + 1 boundaries whose
    differences inside an item are its frames' bytes; item_first_block: n_items + 1, or None for one item that owns every block;
    items: the item of each range, or None for item 0; ranges: (first, count) pairs counted from the item's own first block, or None
    for whole items (then items names them).  -> what plan_cut gives.  Raises TsqError(3) when refused."""
    import numpy as np
    ifb = None if item_first_block is None else np.ascontiguousarray(item_first_block, dtype=np.uint64)
    it = None if items is None else np.array([int(i) for i in items], dtype=np.uint32)
    first = None if ranges is None else np.array([int(f) for f, _ in ranges], dtype=np.uint64)
    count = None if ranges is None else np.array([int(n) for _, n in ranges], dtype=np.uint64)
    if ranges is None and items is None:
        raise TsqError(3, "tsqa_plan_cut_items: neither items nor ranges")
    return _plan_cut("tsqa_plan_cut_items", frame_at, out_start, (ifb, 1 if ifb is None else len(ifb) - 1, it, first, count),
                     len(first) if first is not None else len(it), align, out_size)


def plan_gather(out_start, item_first_block, items, offsets, lengths, align: int = 1, out_cap=None, cap_pieces=None):
    """tsqa_plan_gather (host only): the layout and the verdicts of a gather of the ranges [offsets[k], offsets[k] + lengths[k]) --
    of item items[k]'s data, or of the whole data when items is None -- out of an index with these block starts (out_start, as
    plan_ranges takes it) and first blocks per item (item_first_block, as plan_item_ranges takes it; [0, n_blocks] for one
    container).  out_cap / cap_pieces None: no limit, which sizes a call.  -> (out_offsets, then the bytes needed; range_status: 0,
    3 for a refused range, 6 for an accepted one that does not fit; the pieces the accepted ranges need; the blocks the fitting
    ranges touch).  Raises TsqError(3) when the arguments are refused."""
    import numpy as np
    u64 = lambda v: np.ascontiguousarray(np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in v], dtype=np.uint64))
    starts, first, off, ln = u64(out_start), u64(item_first_block), u64(offsets), u64(lengths)
    it = None if items is None else np.ascontiguousarray(np.array([int(x) & 0xFFFFFFFF for x in items], dtype=np.uint32))
    n = len(off)
    if len(ln) != n or (it is not None and len(it) != n) or len(starts) < 1 or len(first) < 2:
        raise TsqError(3, "tsqa_plan_gather takes as many lengths (and items) as offsets, n_blocks + 1 block starts and n_items + 1 first blocks")
    out_offsets, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.int32)
    pieces, groups = C.c_uint64(0), C.c_uint32(0)
    rc = lib().tsqa_plan_gather(starts.ctypes.data, len(starts) - 1, first.ctypes.data, len(first) - 1, None if it is None else it.ctypes.data,
                                off.ctypes.data, ln.ctypes.data, n, align, 0xFFFFFFFFFFFFFFFF if out_cap is None else int(out_cap),
                                0xFFFFFFFF if cap_pieces is None else int(cap_pieces), out_offsets.ctypes.data, status.ctypes.data,
                                C.byref(pieces), C.byref(groups))
    if rc:
        raise TsqError(rc, "tsqa_plan_gather refused the arguments")
    return [int(x) for x in out_offsets], [int(x) for x in status[:n]], int(pieces.value), int(groups.value)


ROWS_TRUNCATE = 1                    # TSQA_ROWS_TRUNCATE


def plan_gather_rows(out_start, item_first_block, items, offsets, lengths, row_stride: int, truncate: bool = False, cap_pieces=None, n_rows=None):
    """tsqa_plan_gather_rows (host only): the verdicts of a gather into rows of row_stride bytes, on host tables as plan_gather
    takes them; items, offsets and lengths may each be None (n_rows says how many rows when all are).  cap_pieces None: no limit.
    -> (row_lengths, row_status, [pieces needed, largest accepted length], blocks the delivered rows touch).  Raises TsqError(3)
    when the arguments are refused."""
    import numpy as np
    u64 = lambda v: None if v is None else np.ascontiguousarray(np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in v], dtype=np.uint64))
    starts, first, off, ln = u64(out_start), u64(item_first_block), u64(offsets), u64(lengths)
    it = None if items is None else np.ascontiguousarray(np.array([int(x) & 0xFFFFFFFF for x in items], dtype=np.uint32))
    tables = [t for t in (it, off, ln) if t is not None]
    n = len(tables[0]) if tables else int(n_rows or 0)
    if any(len(t) != n for t in tables) or len(starts) < 1 or len(first) < 2:
        raise TsqError(3, "tsqa_plan_gather_rows takes tables of one length, n_blocks + 1 block starts and n_items + 1 first blocks")
    row_lengths, status, need = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.int32), np.zeros(2, dtype=np.uint64)
    groups = C.c_uint32(0)
    ptr = lambda t: None if t is None else t.ctypes.data
    rc = lib().tsqa_plan_gather_rows(starts.ctypes.data, len(starts) - 1, first.ctypes.data, len(first) - 1, ptr(it), ptr(off), ptr(ln), n,
                                     int(row_stride), ROWS_TRUNCATE if truncate else 0, 0xFFFFFFFF if cap_pieces is None else int(cap_pieces),
                                     row_lengths.ctypes.data, status.ctypes.data, need.ctypes.data, C.byref(groups))
    if rc:
        raise TsqError(rc, "tsqa_plan_gather_rows refused the arguments")
    return [int(x) for x in row_lengths[:n]], [int(x) for x in status[:n]], [int(x) for x in need], int(groups.value)


class ItemRange(C.Structure):
    """tsqa_item_range: bytes [offset, offset + length) of item `item`'s own data -> d_out + out_at"""
    _fields_ = [("item", C.c_uint32), ("pad", C.c_uint32), ("offset", C.c_uint64), ("length", C.c_uint64), ("out_at", C.c_uint64)]


class BlockGroup(C.Structure):
    """tsqa_block_group: block `block` is decoded once, up to `hi`, for the range items [first, first + count)"""
    _fields_ = [("block", C.c_uint32), ("first", C.c_uint32), ("count", C.c_uint32), ("hi", C.c_uint32)]


def _item_range_array(ranges):
    """(item, offset, length, out_at) quadruples -> a ctypes tsqa_item_range array"""
    arr = (ItemRange * max(len(ranges), 1))()
    for k, (item, off, ln, at) in enumerate(ranges):
        arr[k] = ItemRange(int(item), 0, int(off), int(ln), int(at))
    return arr


def plan_item_ranges(out_start, item_first_block, ranges, out_cap: int, cap_items=None, cap_groups=None):
    """tsqa_plan_item_ranges (host only): out_start as for plan_ranges; item_first_block = each item's first block, then the block
    count; ranges = (item, offset, length, out_at).  -> (range items (block, lo, hi, out_at) sorted by (block, lo), groups
    (block, first, count, hi), one per touched block).  Raises TsqError(3) when the call is refused; .needed then holds the counts
    the library reported (None when it reported none)."""
    import numpy as np
    starts = np.ascontiguousarray(out_start, dtype=np.uint64)
    first = np.ascontiguousarray(item_first_block, dtype=np.uint64)
    rr = _item_range_array(ranges)
    ni, ng = C.c_uint32(0xFFFFFFFF), C.c_uint32(0xFFFFFFFF)

    def call(items, ci, groups, cg):
        return lib().tsqa_plan_item_ranges(starts.ctypes.data, starts.size - 1, first.ctypes.data, first.size - 1, rr, len(ranges), out_cap,
                                           items, ci, C.byref(ni), groups, cg, C.byref(ng))

    def refuse(rc):
        e = TsqError(rc, "tsqa_plan_item_ranges refused the ranges")
        e.needed = None if ni.value == 0xFFFFFFFF else (ni.value, ng.value)
        return e

    if cap_items is None or cap_groups is None:
        rc = call(None, 0, None, 0)
        if rc and (ni.value == 0xFFFFFFFF or (ni.value == 0 and ng.value == 0)):
            raise refuse(rc)
        cap_items = ni.value if cap_items is None else cap_items
        cap_groups = ng.value if cap_groups is None else cap_groups
        ni.value = ng.value = 0xFFFFFFFF
    items = (RangeItem * max(cap_items, 1))()
    groups = (BlockGroup * max(cap_groups, 1))()
    rc = call(items, cap_items, groups, cap_groups)
    if rc:
        raise refuse(rc)
    return ([(items[k].block, items[k].lo, items[k].hi, items[k].out_at) for k in range(ni.value)],
            [(groups[k].block, groups[k].first, groups[k].count, groups[k].hi) for k in range(ng.value)])


class BatchIndex(RangeIndex):
    """One index over a batch of .tsq containers in one arena (tsqa_index_create_batch), for reads addressed by item: a block that
    several ranges of a call touch is decoded once.  Refused containers are reported per item (item_status) and cannot be read; the
    inherited flat reads (read_into / read_many with offsets) address the concatenation of the healthy items' data.  Holds a
    reference to the arena, which must not change while the index is used."""

    def __init__(self, codec: "DeviceCodec", arena, spans):
        self.codec, self.blob, self.L = codec, arena, codec.L
        self.h = C.c_void_p()
        codec.torch.cuda.current_stream(codec.device).synchronize()
        status = (C.c_int32 * len(spans))()
        rc = self.L.tsqa_index_create_batch(codec.h, arena.data_ptr(), arena.numel(), _batch_array([(a, n, 0, 0) for a, n in spans]),
                                            len(spans), C.byref(self.h), status)
        if not self.h:
            raise codec._err(rc)
        self.n_blocks = int(self.L.tsqa_index_blocks(self.h))
        self.total = int(self.L.tsqa_index_total(self.h))
        self.items = int(self.L.tsqa_index_items(self.h))
        self.worst_status = rc

    @property
    def cut(self):
        # (RangeIndex.cut takes block ranges of ONE container; hasattr(batch_index, "cut") stays False, as callers may test it)
        raise AttributeError("a BatchIndex has no cut of block ranges alone: cut_items names the item of every range")

    def cut_items(self, d_items, d_first=None, d_count=None, align: int = 16, out=None) -> "PackedBatch":
        """The take: item d_items[k] of the batch -- an int32 CUDA tensor, read as unsigned, or a list of ints -- or, with d_first
        and d_count (int64 CUDA tensors), the blocks [d_first[k], d_first[k] + d_count[k]) of that item counted from its own first
        block, each as a .tsq container of its own, packed in one arena at multiples of `align` (DeviceCodec.cut_items_async: the
        frames are copied, nothing is decoded; items may repeat).  A DeviceBatchIndex takes it before fetch().  Without `out` the
        take is measured first and an arena of exactly the bytes needed is made.  -> a PackedBatch as RangeIndex.cut gives, with the
        device tables (d_offsets, d_sizes) beside the host's.  A nonzero status raises TsqError with the item statuses in the text
        and in .item_status -- 3 for an item that does not exist, was refused or has no such blocks --; for an `out` that is too
        small (6) .needed = the bytes a retry needs."""
        codec, torch = self.codec, self.codec.torch
        if not hasattr(d_items, "data_ptr"):
            import numpy as np
            d_items = torch.from_numpy(np.array([int(i) for i in d_items], dtype=np.uint32).view(np.int32)).to(codec.device)
        n = int(d_items.numel())
        for name, t, dtypes in (("d_items", d_items, (torch.int32, getattr(torch, "uint32", torch.int32))), ("d_first", d_first, (torch.int64,)),
                                ("d_count", d_count, (torch.int64,))):
            if t is not None and (t.dtype not in dtypes or t.device != codec.device or not t.is_contiguous() or t.numel() != n):
                raise TsqError(3, f"{name} must be a contiguous {str(dtypes[0])[6:]} tensor of {n} entries on the codec's device")
        if n == 0 or (d_first is None) != (d_count is None):
            raise TsqError(3, "cut_items: no items, or only one of d_first and d_count")
        batch, d_offsets, d_sizes = _cut_packed(
            codec, "cut_items", n, out, lambda room, *tables: codec.cut_items_async(self, d_items, d_first, d_count, n, align, room, *tables))
        batch.d_offsets, batch.d_sizes = d_offsets, d_sizes
        return batch

    def item_total(self, i: int) -> int:
        return int(self.L.tsqa_index_item_total(self.h, i))

    def item_status(self, i: int) -> int:
        return int(self.L.tsqa_index_item_status(self.h, i))

    def gather(self, d_items, d_offsets, d_lengths, align: int = 1, out=None, cap_pieces=None, range_status: bool = False):
        """RangeIndex.gather addressed by item: range k is bytes [d_offsets[k], d_offsets[k] + d_lengths[k]) of item d_items[k]'s
        own data (d_items: an int32 CUDA tensor, read as unsigned; None: offsets into the concatenation of the healthy items)."""
        return self._gather(d_items, d_offsets, d_lengths, align, out, cap_pieces, range_status)

    def gather_rows(self, d_items, d_offsets=None, d_lengths=None, row_stride: int = 0, pad: int = 0, truncate: bool = False, out=None,
                    cap_pieces=None, row_status: bool = False):
        """RangeIndex.gather_rows addressed by item: row k is bytes [d_offsets[k], d_offsets[k] + d_lengths[k]) of item d_items[k]'s
        own data.  With both tables None every row is a whole item, and with truncate=True the first row_stride bytes of it."""
        return self._gather_rows(d_items, d_offsets, d_lengths, row_stride, pad, truncate, out, cap_pieces, row_status)

    def read_items_into(self, ranges, out, sync: bool = True) -> None:
        """The raw call: ranges = (item, offset, length, out_at), bytes land at out[out_at:].  sync=False: on the current stream,
        nothing waited for, the status in codec.status()."""
        rr = _item_range_array(ranges)
        if sync:
            rc = self.L.tsqa_decompress_item_ranges(self.codec.h, self.h, rr, len(ranges), out.data_ptr(), out.numel(), self.codec._stream())
        else:
            rc = self.L.tsqa_decompress_item_ranges_async(self.codec.h, self.h, rr, len(ranges), out.data_ptr(), out.numel(),
                                                          self.codec._status.data_ptr(), self.codec._stream())
        if rc:
            raise self.codec._err(rc)

    def read(self, item: int, offset: int, length: int, out=None):
        """Bytes [offset, offset + length) of item `item`'s data -> a uint8 CUDA tensor (out[:length] when out is given)."""
        out = self._out(out, length)
        self.read_items_into([(item, offset, length, 0)], out)
        return out[:length]

    def _packed_items(self, ranges, out):
        at, quads = 0, []
        for item, off, ln in ranges:
            quads.append((item, off, ln, at))
            at += int(ln)
        out = self._out(out, at)
        return quads, out, at, [out[a:a + int(ln)] for (_, _, ln, a) in quads]

    def read_many(self, ranges, out=None):
        """One call for many (item, offset, length) ranges, packed back to back.  -> (packed tensor, per-range views into it)."""
        quads, out, n, views = self._packed_items(ranges, out)
        self.read_items_into(quads, out)
        return out[:n], views

    def read_many_async(self, ranges, out=None):
        """read_many on the current torch stream, nothing waited for: the status lands in codec.status()."""
        quads, out, n, views = self._packed_items(ranges, out)
        self.read_items_into(quads, out, sync=False)
        return out[:n], views

    def read_flat_many(self, ranges, out=None):
        """RangeIndex.read_many on the concatenation of the healthy items' data: (offset, length) ranges."""
        return RangeIndex.read_many(self, ranges, out)


def plan_index_packed(blocks, totals, head_status, walk_status, cap_blocks: int):
    """tsqa_plan_index_packed (host only): the fit and the close-up of DeviceCodec.index_packed_async from host tables -- per item
    the header's block count and total, the verdict of the header (and, sized form, table) check, and the walk's verdict.
    -> (item_first (n + 1), item_at (n), item_status (n), [live blocks, total, blocks needed], status)"""
    import numpy as np
    n = len(blocks)
    nb = np.ascontiguousarray(blocks, dtype=np.uint32)
    tot = np.ascontiguousarray(totals, dtype=np.uint64)
    hs = np.ascontiguousarray(head_status, dtype=np.int32)
    ws = np.ascontiguousarray(walk_status, dtype=np.int32)
    first, at, st, words, worst = (C.c_uint64 * (n + 1))(), (C.c_uint64 * max(n, 1))(), (C.c_int32 * max(n, 1))(), (C.c_uint64 * 3)(), C.c_int32(0)
    rc = lib().tsqa_plan_index_packed(nb.ctypes.data, tot.ctypes.data, hs.ctypes.data, ws.ctypes.data, n, int(cap_blocks), first, at, st, words,
                                      C.byref(worst))
    if rc:
        raise TsqError(rc, "plan_index_packed: no items, cap_blocks 0, or an accepted item without blocks or with more bytes than its blocks hold")
    return list(first), list(at)[:n], list(st)[:n], list(words), int(worst.value)


class _DeviceWords:
    """n words at a device address that somebody else owns, for torch.as_tensor: no copy is made.  (torch takes no read-only
    view: the tables are the index's, and nobody writes to them.)"""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (int(ptr), False), "version": 2}


class DeviceBatchIndex(BatchIndex):
    """A BatchIndex made on the device from a packed batch's arena and tables (tsqa_index_create_packed_async): on the current
    stream, nothing read on the host and nothing waited for.  gather() works at once, in both addressing modes; d_item_first
    (int64, items + 1), d_item_status (int32) and d_blocks_total (int64: the live blocks, the total, the blocks of all accepted
    items) are the index's own device tables as tensors, to be read behind the creation; they live as long as the index.  Until
    fetch() the host knows nothing: n_blocks and total are 0, item_total gives 0, item_status 3, and the reads the host plans
    (read, read_many, read_flat_many) raise TsqError(3).  Holds references to the arena and the tables."""

    def __init__(self, codec: "DeviceCodec", arena, d_offsets, d_sizes, n_items: int, cap_blocks: int, block_len=None, d_table_first=None,
                 d_block_sizes=None):
        torch = codec.torch
        self.codec, self.blob, self.L = codec, arena, codec.L
        self.tables = (d_offsets, d_sizes, d_table_first, d_block_sizes)
        self.h = C.c_void_p()
        n_items, cap_blocks = int(n_items), int(cap_blocks)
        for name, t, dtype, least in (("d_offsets", d_offsets, torch.int64, n_items), ("d_sizes", d_sizes, torch.int64, n_items),
                                      ("d_table_first", d_table_first, torch.int64, n_items + 1), ("d_block_sizes", d_block_sizes, torch.int32, 0)):
            if t is not None and (t.dtype != dtype or t.device != codec.device or not t.is_contiguous() or t.numel() < least):
                raise TsqError(3, f"{name} must be a contiguous {str(dtype)[6:]} tensor of at least {least} entries on the codec's device")
        if (d_block_sizes is None) != (d_table_first is None) or (d_block_sizes is None) != (block_len is None):
            raise TsqError(3, "the sized form takes block_len, d_table_first and d_block_sizes together")
        sized = d_block_sizes is not None
        # (an empty table has no address to give; the call reads no word of it)
        table = d_block_sizes if not sized or d_block_sizes.numel() else torch.zeros(1, dtype=torch.int32, device=codec.device)
        self.d_item_status = torch.empty(max(n_items, 1), dtype=torch.int32, device=codec.device)[:n_items]
        rc = self.L.tsqa_index_create_packed_async(codec.h, arena.data_ptr(), arena.numel(), d_offsets.data_ptr(), d_sizes.data_ptr(), n_items,
                                                   cap_blocks, int(block_len) if sized else 0, d_table_first.data_ptr() if sized else None,
                                                   table.data_ptr() if sized else None, d_block_sizes.numel() if sized else 0, C.byref(self.h),
                                                   self.d_item_status.data_ptr(), codec._status.data_ptr(), codec._stream())
        if rc:
            raise codec._err(rc)
        first, words = C.c_void_p(), C.c_void_p()
        self.L.tsqa_index_device_tables(self.h, C.byref(first), None, C.byref(words))
        self.d_item_first = torch.as_tensor(_DeviceWords(first.value, n_items + 1, "<i8"), device=codec.device)
        self.d_blocks_total = torch.as_tensor(_DeviceWords(words.value, 3, "<i8"), device=codec.device)
        self.n_blocks, self.total, self.items, self.cap_blocks, self.fetched = 0, 0, n_items, cap_blocks, False
        self.worst_status = None

    def close(self):
        self.d_item_first = self.d_blocks_total = None      # (views of the index's own memory)
        BatchIndex.close(self)

    def fetch(self) -> "DeviceBatchIndex":
        """tsqa_index_fetch: the tables and descriptors come to the host behind the current stream's work, which is waited for.
        From then on this is a BatchIndex in every respect (item statuses may also read 3 or 6).  -> self"""
        rc = self.L.tsqa_index_fetch(self.codec.h, self.h, self.codec._stream())
        if rc:
            raise self.codec._err(rc)
        self.n_blocks = int(self.L.tsqa_index_blocks(self.h))
        self.total = int(self.L.tsqa_index_total(self.h))
        self.worst_status = max(self.item_status(i) for i in range(self.items))
        self.fetched = True
        return self


class PackedBatch:
    """What DeviceCodec.compress_batch_packed gives: the containers of a batch one after the other in a dense arena.
    arena: the used bytes (offsets[-1] of them); offsets (n + 1) and sizes (n): host ints, container i = arena[offsets[i]:offsets[i] +
    sizes[i]] = views[i]; lengths: the items' uncompressed sizes.  A batch of short blocks (compress_batch_packed(..., block_len=))
    also carries block_len, first_block (host ints, n + 1) and d_block_sizes (an int32 CUDA tensor): d_block_sizes[first_block[i]:
    first_block[i + 1]] is the table that decompress_sized and index_sized take for views[i]; all three are None otherwise."""

    def __init__(self, codec: "DeviceCodec", arena, offsets, sizes, lengths, block_len=None, d_block_sizes=None, first_block=None):
        self.codec, self.arena, self._host = codec, arena, (offsets, sizes, lengths)
        self.block_len, self.d_block_sizes, self.first_block = block_len, d_block_sizes, first_block
        # the tables in device memory, where the batch came with them (from_device); d_first_block: of a batch of short blocks
        self.d_offsets = self.d_sizes = self.d_first_block = None
        self._views = None
        self._take_index = None                              # the device index that take() makes and keeps
        # the blocks of all items, where the host knows them: from first_block, from the plain compress (4 MiB blocks), or from the
        # headers once a batch from from_device has been measured; None otherwise (a cut's arena)
        self.n_blocks = first_block[-1] if first_block else None

    def _tables(self):
        """The host tables.  A batch made by from_device measures its headers on the device when they are first asked for, and
        waits for them."""
        if self._host is None:
            codec, n = self.codec, int(self.d_sizes.numel())
            tables = codec._dense_tables(n)
            codec._join()
            codec.decompress_batch_packed_dense_async(self.arena, self.d_offsets, self.d_sizes, n, 0, 1, None, *tables)
            codec._join()
            # (align 1: the differences of the places are the totals)
            host = codec.torch.cat([self.d_offsets[:n], self.d_sizes[:n], tables[0][1:] - tables[0][:-1], tables[2][n:]]).cpu().tolist()
            offsets, sizes, lengths = host[:n], host[n:2 * n], host[2 * n:3 * n]
            if self.n_blocks is None:
                self.n_blocks = host[3 * n]                  # (the accepted headers' block counts)
            self._host = (offsets + [max(o + z for o, z in zip(offsets, sizes))], sizes, lengths)
        return self._host

    offsets = property(lambda self: self._tables()[0])
    sizes = property(lambda self: self._tables()[1])
    lengths = property(lambda self: self._tables()[2])

    @property
    def views(self):
        if self._views is None:
            self._views = [self.arena[o:o + n] for o, n in zip(self.offsets, self.sizes)]
        return self._views

    @classmethod
    def from_device(cls, codec: "DeviceCodec", arena, d_offsets, d_sizes) -> "PackedBatch":
        """A packed batch received as an arena and its two tables in device memory (int64 CUDA tensors: a place per item; one more
        entry in d_offsets is ignored), from whoever made them: no host lengths are needed.  Nothing is read here: index(sync=False)
        works from the device tables alone.  When offsets, sizes, lengths or views are first asked for -- decompress() and index()
        ask --, the headers are measured on the device (DeviceCodec.decompress_batch_packed_dense_async without an output) and
        both tables and the measured sizes come to the host, so that those work as for a batch compressed here; an item whose
        header is refused has length 0 and is refused again by them (a place outside the arena makes tsqa_decompress_batch refuse
        the call).  The tables must not change before that.  To decompress only, DeviceCodec.decompress_packed needs none of this
        and takes such places too."""
        if int(d_sizes.numel()) < 1 or int(d_offsets.numel()) < int(d_sizes.numel()):
            raise TsqError(3, "from_device: no items, or fewer places than sizes")
        self = cls(codec, arena, None, None, None)
        self._host, self.d_offsets, self.d_sizes = None, d_offsets, d_sizes
        return self

    def decompress(self, out=None, item_status: bool = False):
        """The items back, through tsqa_decompress_batch (which decodes again by itself after TSQA_ERR_STALL): a list of views into
        one output arena (`out`, or a new one of sum(lengths) bytes).  item_status=True: a refused item does not raise; -> (views,
        statuses), the view None and the status a TSQA_ERR_* where an item was refused, every healthy item delivered."""
        codec, items, at = self.codec, [], 0
        for o, n, ln in zip(self.offsets, self.sizes, self.lengths):
            items.append((o, n, at, ln))
            at += ln
        out = codec._out_arena(out, at)
        got = (C.c_uint64 * len(items))()
        status = (C.c_int32 * len(items))(*([-1] * len(items))) if item_status else None
        rc = codec.L.tsqa_decompress_batch(codec.h, self.arena.data_ptr(), self.arena.numel(), _batch_array(items), len(items), out.data_ptr(),
                                           out.numel(), got, status, codec._stream())
        # (a return value that is no item's status is an error of the call itself: bad arguments, the HIP runtime)
        if rc and (status is None or rc != max(status)):
            raise codec._err(rc)
        views = [out[a:a + int(got[k])] for k, (_, _, a, _) in enumerate(items)]
        if status is None:
            return views
        return [v if st == 0 else None for v, st in zip(views, status)], [int(st) for st in status]

    def index(self, sync: bool = True, cap_blocks=None):
        """One index over the dense arena, for record reads: index().read(item, offset, length).  sync=False: a DeviceBatchIndex made
        on the current stream from the tables in device memory (DeviceCodec.index_packed_async), nothing waited for; the sized form
        where the batch carries d_block_sizes.  cap_blocks (sync=False only): the blocks the index may hold; by default the batch's
        own count (n_blocks) where the host knows it.  A batch from from_device that has not been measured, or a cut's arena, has
        no count on the host, and the only bound there is -- the arena's bytes in frames of six -- would allocate several times
        the arena: there cap_blocks must be given (TsqError 3 without it; the d_first_block[n] of the compress, or any bound the
        caller knows)."""
        if sync:
            return BatchIndex(self.codec, self.arena, list(zip(self.offsets, self.sizes)))
        codec, torch = self.codec, self.codec.torch
        i64 = lambda values: torch.tensor(values, dtype=torch.int64, device=codec.device)
        if self.d_offsets is None:
            self.d_offsets, self.d_sizes = i64(self.offsets), i64(self.sizes)
        n = int(self.d_sizes.numel())
        sized = self.d_block_sizes is not None
        if sized and self.d_first_block is None:
            self.d_first_block = i64(self.first_block)
        if cap_blocks is None:
            if self.n_blocks is None:
                raise TsqError(3, "index(sync=False): the host does not know this batch's block count (a batch from from_device that has "
                                  "not been measured, or a cut's arena): pass cap_blocks; asking a from_device batch for its lengths "
                                  "measures it, and waits")
            cap_blocks = self.n_blocks
        return codec.index_packed_async(self.arena, self.d_offsets, self.d_sizes, n, max(int(cap_blocks), 1), self.block_len if sized else None,
                                        self.d_first_block if sized else None, self.d_block_sizes)

    def crc32(self, blocks: bool = False, all: bool = True, sync: bool = True) -> "CrcTable":
        """zlib's CRC-32 of every item of the batch, through its index (index().crc32): nothing is decoded into memory."""
        return self.index().crc32(blocks=blocks, all=all, sync=sync)

    def take(self, d_items, align: int = 16, out=None, sync: bool = True) -> "PackedBatch":
        """The items d_items[k] of this batch (an int32 CUDA tensor, read as unsigned, or a list of ints; in any order, with
        repeats) as a new packed batch: BatchIndex.cut_items of whole items through the batch's device index, which is made on the
        current stream when it is first needed (index(sync=False), with cap_blocks as that chooses it: a batch whose block count
        the host does not know takes through an index of its own making, index(sync=False, cap_blocks=...).cut_items).  Nothing is decoded.
        sync=False: nothing is waited for and nothing read on the host.  The output is `out`, or a new arena with room for every
        selection without repeats (the source arena's bytes and align - 1 per item); -> a PackedBatch.from_device over it, with
        .d_item_status (int32: 3 for an item that does not exist or was refused, 6 for one that did not fit), .d_totals and
        d_offsets[n] = the room a retry needs; the largest item status lands in codec.status()."""
        codec, torch = self.codec, self.codec.torch
        if self._take_index is None:
            self._take_index = self.index(sync=False)
        index = self._take_index
        if sync:
            return index.cut_items(d_items, align=align, out=out)
        if not hasattr(d_items, "data_ptr"):
            import numpy as np
            d_items = torch.from_numpy(np.array([int(i) for i in d_items], dtype=np.uint32).view(np.int32)).to(codec.device)
        n = int(d_items.numel())
        if n == 0:
            raise TsqError(3, "take: no items")
        if out is None:
            out = torch.empty(max(int(self.arena.numel()) + n * (int(align) - 1), 16), dtype=torch.uint8, device=codec.device)
        i64 = lambda k: torch.empty(k, dtype=torch.int64, device=codec.device)
        d_offsets, d_sizes, d_totals, d_status = i64(n + 1), i64(n), i64(n), torch.empty(n, dtype=torch.int32, device=codec.device)
        codec.cut_items_async(index, d_items, None, None, n, align, out, d_offsets, d_sizes, d_totals, d_status)
        batch = PackedBatch.from_device(codec, out, d_offsets, d_sizes)
        batch.d_item_status, batch.d_totals = d_status, d_totals
        return batch

    def join(self, out=None, block_sizes: bool = False):
        """The batch as ONE .tsq container whose data is the concatenation of the items' data (DeviceCodec.join of the views:
        the arena is read in place, nothing is decoded).  -> the container trimmed to its size; block_sizes=True: -> (container,
        the table of stream lengths that decompress_sized takes)."""
        return self.codec.join(self.views, out=out, block_sizes=block_sizes)


DONE_FN = C.CFUNCTYPE(None, C.c_uint32, C.c_bool, C.c_void_p)
PROGRESS_FN = C.CFUNCTYPE(None, C.c_uint32, C.c_double, C.c_void_p)
_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def container_bound(n: int) -> int:
    return int(lib().tsqa_container_bound(n))


class DeviceCodec:
    """Device-resident compress/decompress over torch uint8 CUDA tensors (tsqa_* C ABI)."""

    def __init__(self, device: int = -1, ab=False):
        import torch
        if not torch.cuda.is_available():
            raise TsqError(1, "torch sees no GPU")
        self.torch = torch
        self.L = lib(ab)
        self.h = C.c_void_p()
        if device < 0:
            device = torch.cuda.current_device()
        rc = self.L.tsqa_create(device, C.byref(self.h))
        if rc:
            raise TsqError(rc)
        self.device = torch.device("cuda", device)
        self._size = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._status = torch.zeros(1, dtype=torch.int32, device=self.device)

    def close(self):
        if self.h:
            self.L.tsqa_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, rc):
        return TsqError(rc, self.L.tsqa_last_error(self.h).decode())

    def last_error(self) -> str:
        return self.L.tsqa_last_error(self.h).decode()

    def set_variant(self, enc: int, dec: int) -> None:
        self.L.tsqa_set_kernel_variant(self.h, enc, dec)

    def set_decode_wait_limit(self, polls: int) -> None:
        """polls a several-workgroups-per-block decode waits for a sibling workgroup before it reports TSQA_ERR_STALL"""
        self.L.tsqa_set_decode_wait_limit(self.h, polls)

    def profile(self, on: bool) -> None:
        self.L.tsqa_profile_enable(self.h, 1 if on else 0)

    def profile_read(self):
        """-> (encode_ms_sum, encode_launches, decode_ms_sum, decode_launches) since the last read."""
        em, dm, en, dn = C.c_double(0), C.c_double(0), C.c_uint32(0), C.c_uint32(0)
        self.L.tsqa_profile_read(self.h, C.byref(em), C.byref(en), C.byref(dm), C.byref(dn))
        return em.value, en.value, dm.value, dn.value

    def profile_read_calls(self):
        """-> (compress_ms_sum, calls, decompress_ms_sum, calls): whole calls (encode + pack; frame walk + decode)."""
        em, dm, en, dn = C.c_double(0), C.c_double(0), C.c_uint32(0), C.c_uint32(0)
        self.L.tsqa_profile_read_calls(self.h, C.byref(em), C.byref(en), C.byref(dm), C.byref(dn))
        return em.value, en.value, dm.value, dn.value

    def profile_read_join(self):
        """-> (emit_ms_sum, launches): the copy kernel of join_async alone since the last read."""
        ms, n = C.c_double(0), C.c_uint32(0)
        self.L.tsqa_profile_read_join(self.h, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def profile_read_cut(self):
        """-> (emit_ms_sum, launches): the copy kernel of cut_async alone since the last read."""
        ms, n = C.c_double(0), C.c_uint32(0)
        self.L.tsqa_profile_read_cut(self.h, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def profile_read_gather(self):
        """-> (plan_ms_sum, calls, decode_ms_sum, launches): the planner of gather_async, and the decode kernel of the record reads
        (gather_async and BatchIndex.read_items_into) since the last read."""
        pm, pn, dm, dn = C.c_double(0), C.c_uint32(0), C.c_double(0), C.c_uint32(0)
        self.L.tsqa_profile_read_gather(self.h, C.byref(pm), C.byref(pn), C.byref(dm), C.byref(dn))
        return pm.value, pn.value, dm.value, dn.value

    def profile_read_rows(self):
        """-> (pad_ms_sum, launches): the pad kernel of gather_rows_async since the last read (its planner and its decode kernel are
        counted by profile_read_gather)."""
        pm, pn = C.c_double(0), C.c_uint32(0)
        self.L.tsqa_profile_read_rows(self.h, C.byref(pm), C.byref(pn))
        return pm.value, pn.value

    def profile_read_records(self):
        """-> (mark_ms_sum, launches, table_ms_sum, calls): the mark decode of records_async (the decoder that writes one bit per
        byte) and its table launches since the last read."""
        mm, mn, tm, tn = C.c_double(0), C.c_uint32(0), C.c_double(0), C.c_uint32(0)
        self.L.tsqa_profile_read_records(self.h, C.byref(mm), C.byref(mn), C.byref(tm), C.byref(tn))
        return mm.value, mn.value, tm.value, tn.value

    def profile_read_find(self):
        """-> (find_ms_sum, launches, table_ms_sum, calls): the find decode of find_async (the decoder that compares with the
        needle) and its seam and table launches since the last read."""
        fm, fn, tm, tn = C.c_double(0), C.c_uint32(0), C.c_double(0), C.c_uint32(0)
        self.L.tsqa_profile_read_find(self.h, C.byref(fm), C.byref(fn), C.byref(tm), C.byref(tn))
        return fm.value, fn.value, tm.value, tn.value

    def profile_read_crc(self):
        """-> (decode_ms_sum, launches, fold_ms_sum, calls): the CRC decode of crc32_async (the decoder that checksums) and its fold
        and close launches since the last read."""
        dm, dn, fm, fn = C.c_double(0), C.c_uint32(0), C.c_double(0), C.c_uint32(0)
        self.L.tsqa_profile_read_crc(self.h, C.byref(dm), C.byref(dn), C.byref(fm), C.byref(fn))
        return dm.value, dn.value, fm.value, fn.value

    def measure_copy(self, nbytes: int = 1 << 30, reps: int = 7):
        """-> (best, median) GB/s of a plain device copy kernel, bytes read + written."""
        best, med = C.c_double(0), C.c_double(0)
        rc = self.L.tsqa_measure_copy(self.h, nbytes, reps, C.byref(best), C.byref(med))
        if rc:
            raise self._err(rc)
        return best.value, med.value

    def copy_probe_shape(self) -> str:
        """Which launch shape the last measure_copy chose."""
        return self.L.tsqa_copy_probe_shape(self.h).decode()

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    # ---- sharded operation: this device owns some of a job's blocks (tsqa_*_blocks_async) ----
    def encode_blocks_async(self, d_in, n_blocks: int, stride: int, last_len: int, ext: int, d_slots, d_sizes):
        rc = self.L.tsqa_encode_blocks_async(self.h, d_in.data_ptr(), n_blocks, stride, last_len, int(ext), d_slots.data_ptr(),
                                             d_sizes.data_ptr(), self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def decode_blocks_async(self, d_streams, d_frames, n_blocks: int, d_out):
        rc = self.L.tsqa_decode_blocks_async(self.h, d_streams.data_ptr(), d_frames.data_ptr(), n_blocks, d_out.data_ptr(),
                                             self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def frames_to_host_async(self, d_slots, sizes, frame_at, ext: int, host_ptr: int):
        """sizes (uint32) / frame_at (uint64): contiguous numpy arrays, one entry per owned block."""
        rc = self.L.tsqa_frames_to_host_async(self.h, d_slots.data_ptr(), sizes.ctypes.data, frame_at.ctypes.data, len(sizes), int(ext),
                                              host_ptr, self._stream())
        if rc:
            raise self._err(rc)

    def frames_from_host_async(self, host_ptr: int, frame_at, sizes, d_streams):
        rc = self.L.tsqa_frames_from_host_async(self.h, host_ptr, frame_at.ctypes.data, sizes.ctypes.data, len(sizes), d_streams.data_ptr(),
                                                self._stream())
        if rc:
            raise self._err(rc)

    def sharded_place_async(self, d_slots, all_sizes, n_total: int, rank: int, world: int, ext: int, host_ptr: int, host_cap: int) -> int:
        """all_sizes: contiguous numpy uint32, one entry per block of the job.  -> container size."""
        total = C.c_uint64(0)
        rc = self.L.tsqa_sharded_place_async(self.h, d_slots.data_ptr(), all_sizes.ctypes.data, len(all_sizes), n_total, rank, world, int(ext),
                                             host_ptr, host_cap, C.byref(total), self._stream())
        if rc:
            raise self._err(rc)
        return int(total.value)

    def sharded_fetch_decode_async(self, host_ptr: int, container_size: int, rank: int, world: int, d_streams, d_out) -> int:
        """-> the job's uncompressed size (from the container header)."""
        total = C.c_uint64(0)
        rc = self.L.tsqa_sharded_fetch_decode_async(self.h, host_ptr, container_size, rank, world, d_streams.data_ptr(), d_streams.numel(),
                                                    d_out.data_ptr(), d_out.numel(), self._status.data_ptr(), C.byref(total), self._stream())
        if rc:
            raise self._err(rc)
        return int(total.value)

    def sharded_decode_again_async(self, d_streams, d_out) -> None:
        """After status() == 7 (TSQA_ERR_STALL) behind sharded_fetch_decode_async: the owned frames, still on the device, once
        more on one workgroup per block."""
        rc = self.L.tsqa_sharded_decode_again_async(self.h, d_streams.data_ptr(), d_out.data_ptr(), self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def status(self) -> int:
        return int(self._status.item())

    def compress(self, src, ext: int, out=None):
        """src: uint8 CUDA tensor.  Returns a uint8 CUDA tensor view holding the .tsq container."""
        n = src.numel()
        if out is None:
            out = self.torch.empty(container_bound(n), dtype=self.torch.uint8, device=self.device)
        sz = C.c_size_t(0)
        rc = self.L.tsqa_compress_device(self.h, src.data_ptr(), n, out.data_ptr(), out.numel(), C.byref(sz), int(ext), self._stream())
        if rc:
            raise self._err(rc)
        return out[: sz.value]

    def decompress(self, blob, out=None, out_cap=None):
        n = blob.numel()
        if out is None:
            total = int.from_bytes(bytes(blob[8:16].cpu().numpy()), "little") if out_cap is None else out_cap
            out = self.torch.empty(max(total, 1), dtype=self.torch.uint8, device=self.device)
        sz = C.c_size_t(0)
        rc = self.L.tsqa_decompress_device(self.h, blob.data_ptr(), n, out.data_ptr(), out.numel(), C.byref(sz), self._stream())
        if rc:
            raise self._err(rc)
        return out[: sz.value]

    # asynchronous forms: nothing is synchronised; results land in self._size / self._status
    def compress_async(self, src, ext: int, out):
        rc = self.L.tsqa_compress_device_async(self.h, src.data_ptr(), src.numel(), out.data_ptr(), out.numel(),
                                               self._size.data_ptr(), self._status.data_ptr(), int(ext), self._stream())
        if rc:
            raise self._err(rc)

    def decompress_async(self, blob, n_blocks: int, out):
        rc = self.L.tsqa_decompress_device_async(self.h, blob.data_ptr(), blob.numel(), n_blocks, out.data_ptr(), out.numel(),
                                                 self._size.data_ptr(), self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def last_size_status(self):
        return int(self._size.item()), int(self._status.item())

    # ---- short blocks: one container cut every block_len bytes, and the decompress that walks its frames from a size table ----
    def compress_split(self, src, ext: int, block_len: int, out=None, block_sizes: bool = False):
        """compress with blocks of block_len bytes (a power of two from 2^12 to 2^22) instead of 4 MiB: one .tsq container that
        every decode entry point reads, made and read with as many workgroups as it has blocks.  -> the container (a view of `out`,
        or of a new tensor of plan_split's bound); block_sizes=True: -> (container, the blocks' stream lengths: an int32 CUDA tensor,
        one per block, for decompress_sized).  An `out` that is too small raises TsqError(6) with .needed = the bytes a retry needs."""
        n = src.numel()
        nb, bound = plan_split(n, block_len)
        if out is None:
            out = self.torch.empty(bound, dtype=self.torch.uint8, device=self.device)
        table = self.torch.empty(nb, dtype=self.torch.int32, device=self.device) if block_sizes else None
        sz = C.c_size_t(0)
        rc = self.L.tsqa_compress_device_split(self.h, src.data_ptr(), n, int(block_len), out.data_ptr(), out.numel(), C.byref(sz),
                                               table.data_ptr() if block_sizes else None, int(ext), self._stream())
        if rc:
            e = self._err(rc)
            if rc == 6:
                e.needed = int(sz.value)
            raise e
        return (out[: sz.value], table) if block_sizes else out[: sz.value]

    def compress_split_async(self, src, ext: int, block_len: int, out, d_block_sizes=None) -> None:
        """tsqa_compress_device_split_async on the current stream, nothing waited for: the container lands in out, its size and the
        status where compress_async leaves them (last_size_status), the blocks' stream lengths in d_block_sizes (an int32 CUDA
        tensor of plan_split's block count, or None)."""
        if d_block_sizes is not None:
            self._check_table(d_block_sizes, plan_split(src.numel(), block_len)[0], at_least=True)
        rc = self.L.tsqa_compress_device_split_async(self.h, src.data_ptr(), src.numel(), int(block_len), out.data_ptr(), out.numel(),
                                                     self._size.data_ptr(), d_block_sizes.data_ptr() if d_block_sizes is not None else None,
                                                     self._status.data_ptr(), int(ext), self._stream())
        if rc:
            raise self._err(rc)

    def decompress_sized(self, blob, block_sizes, out=None):
        """decompress with the frame walk made in parallel from block_sizes (an int32 CUDA tensor: every block's stream length, as
        compress_split(..., block_sizes=True) gives it).  The table is checked against the container: a false one raises
        TsqError(4), and so does a container whose header states another block count than the table has entries."""
        n = blob.numel()
        self._check_table(block_sizes, None)
        if out is None:
            total = int.from_bytes(bytes(blob[8:16].cpu().numpy()), "little")
            out = self.torch.empty(max(total, 1), dtype=self.torch.uint8, device=self.device)
        sz = C.c_size_t(0)
        rc = self.L.tsqa_decompress_device_sized(self.h, blob.data_ptr(), n, block_sizes.numel(), block_sizes.data_ptr(), out.data_ptr(),
                                                 out.numel(), C.byref(sz), self._stream())
        if rc:
            raise self._err(rc)
        return out[: sz.value]

    def _check_table(self, table, n_blocks, at_least=False):
        """a size table is a contiguous int32 tensor on the codec's device, of n_blocks entries where the count is stated (at_least:
        of no fewer)"""
        if (table.dtype != self.torch.int32 or not table.is_cuda or table.device != self.device or table.dim() != 1 or
                not table.is_contiguous() or table.numel() == 0 or table.numel() >= 1 << 32):
            raise TsqError(3, "block_sizes must be a contiguous 1-D int32 tensor on the codec's device")
        if n_blocks is not None and (table.numel() < n_blocks if at_least else table.numel() != n_blocks):
            raise TsqError(3, f"block_sizes holds {table.numel()} entries, not n_blocks = {n_blocks}")

    def decompress_sized_async(self, blob, n_blocks: int, d_block_sizes, out) -> None:
        """tsqa_decompress_device_sized_async on the current stream, nothing waited for: decompress_async with the table, which
        must hold exactly n_blocks entries."""
        self._check_table(d_block_sizes, n_blocks)
        rc = self.L.tsqa_decompress_device_sized_async(self.h, blob.data_ptr(), blob.numel(), n_blocks, d_block_sizes.data_ptr(), out.data_ptr(),
                                                       out.numel(), self._size.data_ptr(), self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def index(self, blob) -> RangeIndex:
        """An index of the .tsq container `blob` (uint8 CUDA tensor) for range reads: index(blob).read(offset, length)."""
        return RangeIndex(self, blob)

    def index_sized(self, blob, total: int, block_len: int, block_sizes, sync: bool = True) -> SizedIndex:
        """An index of the short-block container `blob` of `total` bytes cut every block_len, from block_sizes (an int32 CUDA
        tensor: what compress_split(..., block_sizes=True) or compress_split_async leaves).  blob may be the whole room the container
        was compressed into.  sync=True waits and raises TsqError(4) for a container that is not what the table and the geometry
        say; sync=False runs on the current torch stream with nothing waited for."""
        return SizedIndex(self, blob, total, block_len, block_sizes, sync)

    def index_packed_async(self, arena, d_offsets, d_sizes, n_items: int, cap_blocks: int, block_len=None, d_table_first=None,
                           d_block_sizes=None) -> DeviceBatchIndex:
        """tsqa_index_create_packed_async on the current stream, nothing waited for and nothing read on the host: one index over the
        containers arena[d_offsets[i]:][:d_sizes[i]] (int64 CUDA tensors, as the packed compress calls leave them).  cap_blocks: the
        blocks the index may hold (it sizes the index and every gather through it: pass a tight value).  Sized form, for a batch
        of short blocks: block_len, d_block_sizes (int32) and d_table_first (int64, n_items + 1: item i's words are
        d_block_sizes[d_table_first[i]:d_table_first[i + 1]], the d_first_block of compress_batch_packed_tables_split_async) make
        the frame walk parallel over the batch's blocks.  -> a DeviceBatchIndex; the largest item status lands in status()."""
        return DeviceBatchIndex(self, arena, d_offsets, d_sizes, n_items, cap_blocks, block_len, d_table_first, d_block_sizes)

    def index_batch(self, blobs) -> "BatchIndex":
        """One index over many .tsq containers (1-D uint8 CUDA tensors), made in one call: index_batch(blobs).read(item, offset,
        length).  Views of one storage are indexed in place; separate allocations are first packed with one torch.cat."""
        arena, offs = self._arena(blobs)
        return BatchIndex(self, arena, [(o, b.numel()) for o, b in zip(offs, blobs)])

    # ---- batches: many independent items in one call (tsqa_*_batch) ----
    def _arena(self, tensors):
        """-> (arena tensor, offset of each tensor in it).  Views of one storage are used in place (the arena is the whole storage);
        separate allocations are packed into a new arena with one torch.cat, a device copy of every byte."""
        torch = self.torch
        if not tensors:
            raise TsqError(3, "a batch needs at least one item")
        for t in tensors:
            if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 1 or not t.is_contiguous() or t.device != self.device:
                raise TsqError(3, "batch items must be contiguous 1-D uint8 tensors on the codec's device")
        st = tensors[0].untyped_storage()
        if all(t.untyped_storage().data_ptr() == st.data_ptr() for t in tensors):
            arena = torch.empty(0, dtype=torch.uint8, device=self.device).set_(st, 0, (st.nbytes(),))
            return arena, [t.data_ptr() - st.data_ptr() for t in tensors]
        offs, at = [], 0
        for t in tensors:
            offs.append(at)
            at += t.numel()
        return torch.cat(tensors), offs

    def _out_arena(self, out, need: int):
        if out is None:
            return self.torch.empty(max(need, 1), dtype=self.torch.uint8, device=self.device)
        if out.dtype != self.torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() < need:
            raise TsqError(3, f"out must be a contiguous uint8 CUDA tensor of at least {need} bytes")
        return out

    def compress_batch(self, srcs, ext: int, out=None):
        """Compress many 1-D uint8 CUDA tensors in one call.  Item i's container is what compress(srcs[i]) gives.  -> a list of views
        into one output arena (`out`, or a new one of sum(batch_bound(n)) bytes), each trimmed to its container.  Views of one
        storage are read in place; separate allocations are first packed with one torch.cat (a device copy)."""
        arena, offs = self._arena(srcs)
        items, at = [], 0
        for o, t in zip(offs, srcs):
            cap = batch_bound(t.numel())
            items.append((o, t.numel(), at, cap))
            at += cap
        out = self._out_arena(out, at)
        sizes = (C.c_uint64 * len(items))()
        rc = self.L.tsqa_compress_batch(self.h, arena.data_ptr(), arena.numel(), _batch_array(items), len(items), int(ext), out.data_ptr(),
                                        out.numel(), sizes, self._stream())
        if rc:
            raise self._err(rc)
        return [out[a:a + int(sizes[k])] for k, (_, _, a, _) in enumerate(items)]

    def compress_batch_packed(self, srcs, ext: int, out=None, align: int = 16, block_len=None) -> PackedBatch:
        """compress_batch into a dense arena: container i starts where container i - 1 ended, rounded up to `align` (a power of two,
        1 to 4096); the places are made on the device once the sizes exist.  -> a PackedBatch whose arena is `out`, or a new tensor
        of the sum(batch_bound(n)) worst case, trimmed to the bytes used.  (The trimmed view keeps the worst-case allocation alive:
        to hold only the used bytes, compress again into an `out` of offsets[-1] bytes.)  An `out` that is too small raises
        TsqError(6) with .needed = the bytes a retry needs.  block_len (a power of two from 2^12 to 2^22): every item is cut into
        blocks of that length, as compress_split cuts one buffer -- container i is compress_split(srcs[i], ext, block_len) --, the
        new arena is made of plan_batch_split's bound, and the batch carries block_len, first_block and d_block_sizes."""
        align = int(align)
        if not 1 <= align <= 4096 or align & (align - 1):
            raise TsqError(3, f"align {align} is not a power of two from 1 to 4096")
        if out is not None and (out.dtype != self.torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.device != self.device):
            raise TsqError(3, "out must be a contiguous uint8 tensor on the codec's device")
        arena, offs = self._arena(srcs)
        items = [(o, t.numel(), 0, 0) for o, t in zip(offs, srcs)]
        if block_len is not None:
            first, bound = plan_batch_split(items, arena.numel(), int(block_len), align)
            if out is None:
                out = self.torch.empty(bound, dtype=self.torch.uint8, device=self.device)
            table = self.torch.empty(first[-1], dtype=self.torch.int32, device=self.device)
            offsets = (C.c_uint64 * (len(items) + 1))()
            sizes = (C.c_uint64 * len(items))()
            rc = self.L.tsqa_compress_batch_packed_split(self.h, arena.data_ptr(), arena.numel(), _batch_array(items), len(items), int(ext), align,
                                                         int(block_len), out.data_ptr(), out.numel(), offsets, sizes, table.data_ptr(),
                                                         self._stream())
            if rc:
                e = self._err(rc)
                if rc == 6:
                    e.needed = int(offsets[len(items)])
                raise e
            offsets = [int(x) for x in offsets]
            return PackedBatch(self, out[:offsets[-1]], offsets, [int(x) for x in sizes], [t.numel() for t in srcs], int(block_len), table, first)
        if out is None:
            worst = sum(batch_bound(t.numel()) for t in srcs) + (len(srcs) - 1) * (align - 1)           # (and the padding between them)
            out = self.torch.empty(worst, dtype=self.torch.uint8, device=self.device)
        offsets = (C.c_uint64 * (len(items) + 1))()
        sizes = (C.c_uint64 * len(items))()
        rc = self.L.tsqa_compress_batch_packed(self.h, arena.data_ptr(), arena.numel(), _batch_array(items), len(items), int(ext), int(align),
                                               out.data_ptr(), out.numel(), offsets, sizes, self._stream())
        if rc:
            e = self._err(rc)
            if rc == 6:
                e.needed = int(offsets[len(items)])
            raise e
        offsets = [int(x) for x in offsets]
        batch = PackedBatch(self, out[:offsets[-1]], offsets, [int(x) for x in sizes], [t.numel() for t in srcs])
        batch.n_blocks = sum(-(-t.numel() // BLOCK_SZ) for t in srcs)
        return batch

    def decompress_batch(self, blobs, out=None):
        """Decompress many .tsq containers (1-D uint8 CUDA tensors) in one call.  -> a list of views into one output arena, each trimmed
        to its item's size.  A refused item raises TsqError with .item_status (one TSQA_ERR_* or 0 per item) and .results (the views,
        None where refused): every healthy item is still delivered."""
        import numpy as np
        arena, offs = self._arena(blobs)
        # every header with one gather and one copy: the output room each item asks for (0 for a header the library will refuse)
        lens = np.array([b.numel() for b in blobs], dtype=np.int64)
        pos = self.torch.tensor(np.minimum(np.array(offs, dtype=np.int64)[:, None] + np.arange(16), arena.numel() - 1), device=self.device)
        heads = arena[pos].cpu().numpy().astype(np.uint64)
        word = lambda lo, n: sum(heads[:, lo + k] << np.uint64(8 * k) for k in range(n))
        magic, nb, total = word(0, 4), word(4, 4), word(8, 8)
        room = (np.maximum(lens, 16) - 16).astype(np.uint64) // np.uint64(6)
        plausible = (lens >= 16) & (magic == 0x31515354) & (nb >= 1) & (nb <= room) & (total <= nb * np.uint64(BLOCK_SZ))
        caps = np.where(plausible, total, 0).astype(np.int64)
        items, at = [], 0
        for o, n, cap in zip(offs, lens.tolist(), caps.tolist()):
            items.append((o, n, at, cap))
            at += cap
        out = self._out_arena(out, at)
        sizes = (C.c_uint64 * len(items))()
        status = (C.c_int32 * len(items))()
        rc = self.L.tsqa_decompress_batch(self.h, arena.data_ptr(), arena.numel(), _batch_array(items), len(items), out.data_ptr(), out.numel(),
                                          sizes, status, self._stream())
        views = [out[a:a + int(sizes[k])] for k, (_, _, a, _) in enumerate(items)]
        if rc:
            e = self._err(rc)
            e.item_status = [int(s) for s in status]
            e.results = [v if s == 0 else None for v, s in zip(views, e.item_status)]
            raise e
        return views

    def compress_batch_async(self, arena, items, ext: int, out, d_sizes) -> None:
        """tsqa_compress_batch_async on the current stream, nothing waited for: items = (in_at, in_len, out_at, out_cap) offsets into the
        uint8 CUDA tensors arena and out; container sizes land in d_sizes (an int64 CUDA tensor, one per item), the status in status()."""
        rc = self.L.tsqa_compress_batch_async(self.h, arena.data_ptr(), arena.numel(), _batch_array(items), len(items), int(ext), out.data_ptr(),
                                              out.numel(), d_sizes.data_ptr(), self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def decompress_batch_async(self, arena, items, n_blocks, out, d_sizes) -> None:
        """tsqa_decompress_batch_async on the current stream: as compress_batch_async, with each container's block count."""
        import numpy as np
        nb = np.ascontiguousarray(n_blocks, dtype=np.uint32)
        rc = self.L.tsqa_decompress_batch_async(self.h, arena.data_ptr(), arena.numel(), _batch_array(items), nb.ctypes.data, len(items),
                                                out.data_ptr(), out.numel(), d_sizes.data_ptr(), self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def decompress_batch_items_async(self, arena, items, n_blocks, out, d_sizes, d_item_status) -> None:
        """tsqa_decompress_batch_items_async on the current stream: decompress_batch_async with a verdict per item.  d_item_status
        (an int32 CUDA tensor, one per item) gets each item's TSQA_ERR_* or 0, d_sizes[i] = 0 where it is not 0, and every other
        item is complete; status() becomes the largest item status."""
        import numpy as np
        nb = np.ascontiguousarray(n_blocks, dtype=np.uint32)
        rc = self.L.tsqa_decompress_batch_items_async(self.h, arena.data_ptr(), arena.numel(), _batch_array(items), nb.ctypes.data, len(items),
                                                      out.data_ptr(), out.numel(), d_sizes.data_ptr(),
                                                      d_item_status.data_ptr() if d_item_status is not None else None,
                                                      self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def compress_batch_packed_async(self, arena, items, ext: int, align: int, out, d_offsets, d_sizes) -> None:
        """tsqa_compress_batch_packed_async on the current stream, nothing waited for: items = (in_at, in_len) offsets into the uint8
        CUDA tensor arena (longer tuples: the rest is ignored); the containers land packed in out, their places in d_offsets (int64
        CUDA tensor, one more than items) and d_sizes (one per item), the status in status()."""
        quads = [(it[0], it[1], 0, 0) for it in items]
        rc = self.L.tsqa_compress_batch_packed_async(self.h, arena.data_ptr(), arena.numel(), _batch_array(quads), len(quads), int(ext), int(align),
                                                     out.data_ptr(), out.numel(), d_offsets.data_ptr(), d_sizes.data_ptr(),
                                                     self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def compress_batch_packed_split_async(self, arena, items, ext: int, align: int, block_len: int, out, d_offsets, d_sizes,
                                          d_block_sizes=None) -> None:
        """tsqa_compress_batch_packed_split_async on the current stream, nothing waited for: compress_batch_packed_async with every
        item cut every block_len bytes; d_block_sizes (an int32 CUDA tensor of plan_batch_split's block count, or None) gets every
        block's stream length, item after item."""
        quads = [(it[0], it[1], 0, 0) for it in items]
        if d_block_sizes is not None:
            self._check_table(d_block_sizes, plan_batch_split(quads, arena.numel(), int(block_len), int(align))[0][-1], at_least=True)
        rc = self.L.tsqa_compress_batch_packed_split_async(self.h, arena.data_ptr(), arena.numel(), _batch_array(quads), len(quads), int(ext),
                                                           int(align), int(block_len), out.data_ptr(), out.numel(), d_offsets.data_ptr(),
                                                           d_sizes.data_ptr(), d_block_sizes.data_ptr() if d_block_sizes is not None else None,
                                                           self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def decompress_batch_packed_async(self, arena, d_offsets, d_sizes, items, n_blocks, out, d_out_sizes) -> None:
        """tsqa_decompress_batch_packed_async on the current stream: the containers' places are read from d_offsets and d_sizes on
        the device (as compress_batch_packed_async left them); items = (out_at, out_cap) offsets into out, n_blocks each container's
        block count; the uncompressed sizes land in d_out_sizes (int64 CUDA tensor), the status in status()."""
        import numpy as np
        nb = np.ascontiguousarray(n_blocks, dtype=np.uint32)
        quads = [(0, 0, it[-2], it[-1]) for it in items]
        rc = self.L.tsqa_decompress_batch_packed_async(self.h, arena.data_ptr(), arena.numel(), d_offsets.data_ptr(), d_sizes.data_ptr(),
                                                       _batch_array(quads), nb.ctypes.data, len(quads), out.data_ptr(), out.numel(),
                                                       d_out_sizes.data_ptr(), self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def decompress_batch_packed_items_async(self, arena, d_offsets, d_sizes, items, n_blocks, out, d_out_sizes, d_item_status) -> None:
        """tsqa_decompress_batch_packed_items_async on the current stream: decompress_batch_packed_async with a verdict per item in
        d_item_status (an int32 CUDA tensor, one per item), as decompress_batch_items_async; a bad place is its item's
        TSQA_ERR_FORMAT."""
        import numpy as np
        nb = np.ascontiguousarray(n_blocks, dtype=np.uint32)
        quads = [(0, 0, it[-2], it[-1]) for it in items]
        rc = self.L.tsqa_decompress_batch_packed_items_async(self.h, arena.data_ptr(), arena.numel(), d_offsets.data_ptr(), d_sizes.data_ptr(),
                                                             _batch_array(quads), nb.ctypes.data, len(quads), out.data_ptr(), out.numel(),
                                                             d_out_sizes.data_ptr(),
                                                             d_item_status.data_ptr() if d_item_status is not None else None,
                                                             self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def _join(self) -> None:
        """Around the asynchronous calls of a synchronous method.  A call given torch's default stream runs on the context's own
        stream, which does not wait for torch's work and which torch's reads do not wait for: there, wait for the device.  On any
        other stream the call is enqueued where the caller's work and the reads behind it are."""
        if self.torch.cuda.current_stream(self.device).cuda_stream == 0:
            self.torch.cuda.synchronize(self.device)

    def _dense_tables(self, n: int):
        """-> (d_out_offsets, d_out_sizes, d_first_block, d_item_status) for n items"""
        i64 = lambda k: self.torch.empty(k, dtype=self.torch.int64, device=self.device)
        return i64(n + 1), i64(n), i64(n + 1), self.torch.empty(n, dtype=self.torch.int32, device=self.device)

    def decompress_batch_packed_dense_async(self, arena, d_offsets, d_sizes, n_items: int, cap_blocks: int, align: int, out, d_out_offsets,
                                            d_out_sizes, d_first_block, d_item_status) -> None:
        """tsqa_decompress_batch_packed_dense_async on the current stream, nothing waited for and nothing about the items taken from
        the host: the containers' places are read from d_offsets and d_sizes (int64 CUDA tensors, as compress_batch_packed_async left
        them), their block counts and sizes from their headers on the device, and item i lands at out[d_out_offsets[i]:][:d_out_sizes[i]]
        (int64 CUDA tensors of n_items + 1 and n_items entries; d_first_block: n_items + 1; d_item_status: int32, n_items).  An
        item that does not fit out or cap_blocks blocks gets TSQA_ERR_OVERFLOW (6) and the tables say what a retry needs.  out None:
        measure only.  The largest item status lands in status()."""
        rc = self.L.tsqa_decompress_batch_packed_dense_async(self.h, arena.data_ptr(), arena.numel(), d_offsets.data_ptr(), d_sizes.data_ptr(),
                                                             int(n_items), int(align), int(cap_blocks),
                                                             out.data_ptr() if out is not None else None, out.numel() if out is not None else 0,
                                                             d_out_offsets.data_ptr(), d_out_sizes.data_ptr(), d_first_block.data_ptr(),
                                                             d_item_status.data_ptr(), self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def join_async(self, arena, d_offsets, d_sizes, n_items: int, cap_blocks: int, out, d_first_block, d_block_sizes, d_item_status) -> None:
        """tsqa_join_async on the current stream, nothing waited for and nothing about the items taken from the host: the containers
        arena[d_offsets[i]:][:d_sizes[i]] (int64 CUDA tensors) become one container in out, whose data is the concatenation of
        theirs.  d_first_block: int64, n_items + 1; d_block_sizes: None, or an int32 CUDA tensor of at least cap_blocks entries that
        gets the joined stream lengths (what decompress_sized_async takes); d_item_status: int32, n_items.  The size and the status
        land where compress_async leaves them (last_size_status).  All or nothing: on any nonzero status out is untouched.  out
        None: measure only."""
        if d_block_sizes is not None:
            self._check_table(d_block_sizes, cap_blocks, at_least=True)
        rc = self.L.tsqa_join_async(self.h, arena.data_ptr(), arena.numel(), d_offsets.data_ptr(), d_sizes.data_ptr(), int(n_items), int(cap_blocks),
                                    out.data_ptr() if out is not None else None, out.numel() if out is not None else 0, self._size.data_ptr(),
                                    d_first_block.data_ptr(), d_block_sizes.data_ptr() if d_block_sizes is not None else None,
                                    d_item_status.data_ptr(), self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def cut_async(self, index, d_first, d_count, n: int, align: int, out, d_offsets, d_sizes, d_totals, d_item_status) -> None:
        """tsqa_cut_async on the current stream, nothing waited for and nothing about the ranges taken from the host: the blocks
        [d_first[k], d_first[k] + d_count[k]) of the container behind `index` (a RangeIndex or SizedIndex made before, on this stream
        where it was made without a wait) become container k of a packed arena in out: out[d_offsets[k]:][:d_sizes[k]], decoding
        to d_totals[k] bytes (int64 CUDA tensors of n + 1, n and n entries; d_totals may be None; d_item_status: int32, n).  A range
        outside the index gets TSQA_ERR_ARG (3), one that does not fit out TSQA_ERR_OVERFLOW (6), and d_offsets[n] is the room a
        retry needs.  out None: measure only.  The largest item status lands in status()."""
        rc = self.L.tsqa_cut_async(self.h, index.h, d_first.data_ptr(), d_count.data_ptr(), int(n), int(align),
                                   out.data_ptr() if out is not None else None, out.numel() if out is not None else 0,
                                   d_offsets.data_ptr(), d_sizes.data_ptr(), d_totals.data_ptr() if d_totals is not None else None,
                                   d_item_status.data_ptr(), self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def cut_items_async(self, index, d_items, d_first, d_count, n: int, align: int, out, d_offsets, d_sizes, d_totals, d_item_status) -> None:
        """tsqa_cut_items_async on the current stream, nothing waited for and nothing about the ranges taken from the host: cut_async
        through ANY index -- a BatchIndex or a DeviceBatchIndex, fetched or not, too -- with the item of range k in d_items[k] (an
        int32 CUDA tensor, read as unsigned; None: item 0, for an index of one item) and d_first / d_count counted from the item's
        own first block (both None: the whole item).  The output tables are cut_async's.  An item that does not exist or was
        refused gets TSQA_ERR_ARG (3) as a range outside its item does.  The largest item status lands in status()."""
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = self.L.tsqa_cut_items_async(self.h, index.h, ptr(d_items), ptr(d_first), ptr(d_count), int(n), int(align), ptr(out),
                                         out.numel() if out is not None else 0, d_offsets.data_ptr(), d_sizes.data_ptr(), ptr(d_totals),
                                         d_item_status.data_ptr(), self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def gather_async(self, index, d_items, d_offsets, d_lengths, n: int, align: int, cap_pieces: int, out, d_out_offsets, d_range_status,
                     d_need_pieces, out_cap=None) -> None:
        """tsqa_gather_async on the current stream, nothing waited for and nothing about the ranges taken from the host: bytes
        [d_offsets[k], d_offsets[k] + d_lengths[k]) (int64 CUDA tensors) of the data behind `index` -- any index; of item d_items[k]
        (an int32 CUDA tensor, read as unsigned) where d_items is given -- land at out[d_out_offsets[k]:], packed at multiples of
        align (d_out_offsets: int64, n + 1; d_range_status: int32, n; d_need_pieces: int64, 1).  A range outside its data gets
        TSQA_ERR_ARG (3); one that does not fit out, or whose pieces -- one per block it touches -- do not fit cap_pieces,
        TSQA_ERR_OVERFLOW (6), and d_out_offsets[n] and d_need_pieces say what a retry needs.  The largest range status lands in
        status().  out_cap: the bytes of out that may be written, all of it when None; 0 measures."""
        rc = self.L.tsqa_gather_async(self.h, index.h, d_items.data_ptr() if d_items is not None else None, d_offsets.data_ptr(),
                                      d_lengths.data_ptr(), int(n), int(align), int(cap_pieces), out.data_ptr(),
                                      out.numel() if out_cap is None else min(int(out_cap), out.numel()),
                                      d_out_offsets.data_ptr(), d_range_status.data_ptr(), d_need_pieces.data_ptr(), self._status.data_ptr(),
                                      self._stream())
        if rc:
            raise self._err(rc)

    def gather_rows_async(self, index, d_items, d_offsets, d_lengths, n: int, row_stride: int, flags: int, pad: int, cap_pieces: int, out,
                          d_row_lengths, d_row_status, d_need) -> None:
        """tsqa_gather_rows_async on the current stream, nothing waited for: the ranges of gather_async -- d_items, d_offsets and
        d_lengths may each be None -- land in rows of row_stride bytes, row k at out[k * row_stride:], its tail filled with `pad`
        (-1: left alone); d_row_lengths (int64, n) = the bytes each row got, d_row_status (int32, n) its verdict, d_need (int64, 2)
        = the pieces a retry needs and the largest accepted length.  flags: ROWS_TRUNCATE or 0.  out None measures.  The largest
        row status lands in status()."""
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = self.L.tsqa_gather_rows_async(self.h, index.h, ptr(d_items), ptr(d_offsets), ptr(d_lengths), int(n), int(row_stride), int(flags),
                                           int(pad), int(cap_pieces), ptr(out), out.numel() if out is not None else 0,
                                           d_row_lengths.data_ptr(), d_row_status.data_ptr(), d_need.data_ptr(), self._status.data_ptr(),
                                           self._stream())
        if rc:
            raise self._err(rc)

    def records_async(self, index, delim: int, flags: int, cap_records: int, d_rec_items, d_rec_offsets, d_rec_lengths, d_item_first_record,
                      d_need, d_status=None) -> None:
        """tsqa_records_async on the current stream, nothing waited for: the records of the data behind `index` for the delimiter
        byte `delim` (flags: RECORDS_KEEP_DELIM | RECORDS_FLAT).  The records numbered below cap_records go to d_rec_items (int32,
        may be None), d_rec_offsets and d_rec_lengths (int64; both None with cap_records 0: the call only measures);
        d_item_first_record (int64, items + 1) and d_need (int64, 2: the count of all records, the largest length) are always
        complete.  The status -- 0, 6 more records than cap_records, 4 a refused sized index, 5 a malformed stream -- lands in
        d_status (int32, 1) or, when None, in status()."""
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = self.L.tsqa_records_async(self.h, index.h, int(delim), int(flags), int(cap_records), ptr(d_rec_items), ptr(d_rec_offsets),
                                       ptr(d_rec_lengths), d_item_first_record.data_ptr(), d_need.data_ptr(),
                                       (self._status if d_status is None else d_status).data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def find_async(self, index, needle, flags: int, cap_hits: int, d_hit_items, d_hit_offsets, d_item_first_hit, d_need, d_status=None) -> None:
        """tsqa_find_async on the current stream, nothing waited for: where `needle` (bytes, 1 .. FIND_MAX_NEEDLE of them) occurs in
        the data behind `index` (flags: FIND_FLAT).  The hits numbered below cap_hits go to d_hit_items (int32, may be None) and
        d_hit_offsets (int64, each hit's first byte; None with cap_hits 0: the call only measures); d_item_first_hit (int64,
        items + 1) and d_need (int64, 1: the count of all hits) are always complete.  The status -- 0, 6 more hits than cap_hits, 4
        a refused sized index, 5 a malformed stream -- lands in d_status (int32, 1) or, when None, in status().  The needle is read
        during the call."""
        ptr = lambda t: t.data_ptr() if t is not None else None
        needle = bytes(needle)
        rc = self.L.tsqa_find_async(self.h, index.h, needle, len(needle), int(flags), int(cap_hits), ptr(d_hit_items), ptr(d_hit_offsets),
                                    d_item_first_hit.data_ptr(), d_need.data_ptr(),
                                    (self._status if d_status is None else d_status).data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def crc32_async(self, index, blocks: bool = False, all: bool = True, stream=None, d_items=None, d_item_status=None, d_blocks=None,
                    d_all=None, d_status=None) -> "CrcTable":
        """tsqa_crc32_async on the current stream (or `stream`, a torch stream), nothing waited for: zlib's CRC-32 of every item of
        `index` -> a CrcTable of CUDA tensors.  all / blocks: the whole data's CRC and one CRC per block are asked for too.  The
        tensors are made here unless given (d_items, d_blocks, d_all: int32, whose bits are the uint32 values; d_item_status,
        d_status: int32; a given d_blocks or d_all is asked for whatever the flags say)."""
        torch = self.torch
        i32 = lambda k: torch.empty(max(int(k), 1), dtype=torch.int32, device=self.device)
        n_items = int(self.L.tsqa_index_items(index.h))
        n_blocks = int(self.L.tsqa_index_blocks(index.h))
        d_items = i32(n_items)[:n_items] if d_items is None else d_items
        d_item_status = i32(n_items)[:n_items] if d_item_status is None else d_item_status
        if d_blocks is None and blocks:
            d_blocks = i32(n_blocks)[:n_blocks]
        if d_all is None and all:
            d_all = i32(1)
        d_status = i32(1) if d_status is None else d_status
        ptr = lambda t: t.data_ptr() if t is not None else None
        s = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        rc = self.L.tsqa_crc32_async(self.h, index.h, 0, d_items.data_ptr(), d_item_status.data_ptr(), ptr(d_blocks), ptr(d_all), d_status.data_ptr(), s)
        if rc:
            raise self._err(rc)
        return CrcTable(index, d_items, d_item_status, d_blocks, d_all, d_status)

    def join(self, blobs, out=None, block_sizes: bool = False):
        """Join .tsq containers (1-D uint8 CUDA tensors; placement as in compress_batch: views of one storage are read in place)
        into ONE container that decodes to the concatenation of their data, at copy speed: nothing is decoded.  The block count
        is measured on the device first (one small read); a new `out` has room for every byte of the items.  -> the container, a
        view of `out` trimmed to its size; block_sizes=True: -> (container, the stream lengths of its blocks: an int32 CUDA tensor
        for decompress_sized).  A refused item raises TsqError(4) with .item_status (one TSQA_ERR_* or 0 per item) and nothing is
        written; an `out` that is too small raises TsqError(6) with .needed = the bytes a retry needs."""
        torch = self.torch
        arena, offs = self._arena(blobs)
        n = len(blobs)
        if out is not None and (out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.device != self.device):
            raise TsqError(3, "out must be a contiguous uint8 tensor on the codec's device")
        places = torch.tensor([offs, [b.numel() for b in blobs]], dtype=torch.int64).to(self.device)
        d_first = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        d_status = torch.empty(n, dtype=torch.int32, device=self.device)

        def refuse(code):
            e = self._err(code)
            e.item_status = d_status.cpu().tolist()
            if code == 6:
                e.needed = int(self._size.item())
            return e

        self._join()
        self.join_async(arena, places[0], places[1], n, 1, None, d_first, None, d_status)      # (the headers only: first_block is complete)
        self._join()
        need_blocks = int(d_first[n].item())
        if need_blocks == 0 or need_blocks >= 1 << 32:
            raise refuse(4 if need_blocks == 0 else 6)
        if out is None:
            out = torch.empty(16 + sum(max(b.numel() - 16, 0) for b in blobs), dtype=torch.uint8, device=self.device)
        table = torch.empty(need_blocks, dtype=torch.int32, device=self.device) if block_sizes else None
        self.join_async(arena, places[0], places[1], n, need_blocks, out, d_first, table, d_status)
        self._join()
        size, status = self.last_size_status()
        if status:
            raise refuse(status)
        return (out[:size], table) if block_sizes else out[:size]

    def compress_batch_packed_tables_async(self, data, d_in_offsets, d_in_sizes, n_items: int, cap_blocks: int, ext: int, align: int, out,
                                           d_offsets, d_sizes, d_first_block, d_bound, d_item_status) -> None:
        """tsqa_compress_batch_packed_tables_async on the current stream, nothing waited for and nothing about the items taken from
        the host: item i is data[d_in_offsets[i]:][:d_in_sizes[i]] (int64 CUDA tensors), its container lands packed in out at
        d_offsets[i] with d_sizes[i] bytes (int64 CUDA tensors of n_items + 1 and n_items entries; d_first_block: n_items + 1;
        d_bound: one entry or None; d_item_status: int32, n_items).  An item whose place lies outside data gets TSQA_ERR_ARG (3), one
        that does not fit cap_blocks blocks or out TSQA_ERR_OVERFLOW (6), and the tables say what a retry needs.  out None: measure
        only.  The largest item status lands in status()."""
        rc = self.L.tsqa_compress_batch_packed_tables_async(self.h, data.data_ptr(), data.numel(), d_in_offsets.data_ptr(), d_in_sizes.data_ptr(),
                                                            int(n_items), int(cap_blocks), int(ext), int(align),
                                                            out.data_ptr() if out is not None else None, out.numel() if out is not None else 0,
                                                            d_offsets.data_ptr(), d_sizes.data_ptr(), d_first_block.data_ptr(),
                                                            d_bound.data_ptr() if d_bound is not None else None, d_item_status.data_ptr(),
                                                            self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def compress_batch_packed_tables_split_async(self, data, d_in_offsets, d_in_sizes, n_items: int, cap_blocks: int, ext: int, align: int,
                                                 block_len: int, out, d_offsets, d_sizes, d_first_block, d_bound, d_block_sizes,
                                                 d_item_status) -> None:
        """tsqa_compress_batch_packed_tables_split_async on the current stream: compress_batch_packed_tables_async with every item
        cut every block_len bytes; d_block_sizes (an int32 CUDA tensor of at least cap_blocks entries, or None) gets the stream
        lengths of the fitting items' blocks, word d_first_block[i] + j for block j of item i."""
        if d_block_sizes is not None and out is not None:
            self._check_table(d_block_sizes, int(cap_blocks), at_least=True)
        rc = self.L.tsqa_compress_batch_packed_tables_split_async(self.h, data.data_ptr(), data.numel(), d_in_offsets.data_ptr(),
                                                                  d_in_sizes.data_ptr(), int(n_items), int(cap_blocks), int(ext), int(align),
                                                                  int(block_len), out.data_ptr() if out is not None else None,
                                                                  out.numel() if out is not None else 0, d_offsets.data_ptr(), d_sizes.data_ptr(),
                                                                  d_first_block.data_ptr(), d_bound.data_ptr() if d_bound is not None else None,
                                                                  d_block_sizes.data_ptr() if d_block_sizes is not None else None,
                                                                  d_item_status.data_ptr(), self._status.data_ptr(), self._stream())
        if rc:
            raise self._err(rc)

    def compress_packed_tables(self, data, d_in_offsets, d_in_sizes, ext: int, align: int = 16, cap_blocks=None, out=None,
                               item_status: bool = False, block_len=None):
        """Compress the items data[d_in_offsets[i]:][:d_in_sizes[i]] (int64 CUDA tensors) into a dense arena.  With cap_blocks or out
        missing the batch is measured on the device first and the two "needed" words come back with one copy: the block count, and
        the room that always holds the arena, of which a new `out` is made (trimmed to the bytes used afterwards).  -> a PackedBatch
        (PackedBatch.from_device); item_status=True: -> (batch, statuses), and a refused or unfit item -- status 3 or 6, size 0 --
        does not raise; without it such an item raises TsqError with the largest item status and .item_status.  block_len: every
        item is cut into blocks of that length (compress_batch_packed's block_len), and the batch carries block_len, first_block
        and d_block_sizes (cap_blocks words)."""
        torch = self.torch
        n = int(d_in_sizes.numel())
        d_offsets, d_sizes, d_first, d_status = self._dense_tables(n)
        d_bound = torch.empty(1, dtype=torch.int64, device=self.device)
        self._join()
        if block_len is not None:
            def run(cap, arena, table):
                self.compress_batch_packed_tables_split_async(data, d_in_offsets, d_in_sizes, n, cap, ext, align, block_len, arena, d_offsets,
                                                              d_sizes, d_first, d_bound, table, d_status)
        else:
            def run(cap, arena, table):
                self.compress_batch_packed_tables_async(data, d_in_offsets, d_in_sizes, n, cap, ext, align, arena, d_offsets, d_sizes, d_first,
                                                        d_bound, d_status)
        if cap_blocks is None or out is None:
            run(0, None, None)
            self._join()
            need_blocks, bound = torch.stack([d_first[n], d_bound[0]]).cpu().tolist()
            if cap_blocks is None:
                cap_blocks = max(need_blocks, 1)
            if out is None:
                out = torch.empty(max(bound, 16), dtype=torch.uint8, device=self.device)
        table = torch.zeros(max(int(cap_blocks), 1), dtype=torch.int32, device=self.device) if block_len is not None else None
        run(cap_blocks, out, table)
        self._join()
        status = d_status.cpu().tolist()
        if any(status) and not item_status:
            e = self._err(max(status))
            e.item_status = status
            raise e
        used = int(d_offsets[n].item())
        batch = PackedBatch.from_device(self, out[:min(used, out.numel())], d_offsets, d_sizes)
        if block_len is not None:
            batch.block_len, batch.d_block_sizes, batch.first_block, batch.d_first_block = int(block_len), table, d_first.cpu().tolist(), d_first
            batch.n_blocks = batch.first_block[-1]
        return (batch, status) if item_status else batch

    def decompress_packed(self, arena, d_offsets, d_sizes, align: int = 16, out=None, item_status: bool = False):
        """The items of a packed batch known only by its arena and device tables: measure on the device, read the two "needed" words
        back with one copy, allocate exactly (or check `out`), decode.  -> a list of views into the output arena, item i at
        round_up(end of item i - 1, align); item_status=True: -> (views, statuses) as PackedBatch.decompress gives them, the view
        None and the status a TSQA_ERR_* where an item was refused; without it a refused item raises TsqError with .item_status and
        .results.  An `out` that is too small raises TsqError(6) with .needed = the bytes a retry needs."""
        torch = self.torch
        n = int(d_sizes.numel())
        tables = self._dense_tables(n)
        self._join()
        self.decompress_batch_packed_dense_async(arena, d_offsets, d_sizes, n, 0, align, None, *tables)
        self._join()
        need_bytes, need_blocks = torch.stack([tables[0][n], tables[2][n]]).cpu().tolist()
        if out is not None and out.numel() < need_bytes:
            e = TsqError(6, f"out holds {out.numel()} bytes, the batch needs {need_bytes}")
            e.needed = need_bytes
            raise e
        out = self._out_arena(out, need_bytes)
        if need_blocks:
            self.decompress_batch_packed_dense_async(arena, d_offsets, d_sizes, n, need_blocks, align, out, *tables)
            self._join()
        host = torch.cat([tables[0][:n], tables[1], tables[3].to(torch.int64)]).cpu().tolist()
        status = host[2 * n:]
        views = [out[a:a + z] if st == 0 else None for a, z, st in zip(host[:n], host[n:2 * n], status)]
        if item_status:
            return views, status
        if any(status):
            e = self._err(max(status))
            e.item_status, e.results = status, views
            raise e
        return views


# ---------------------------------------------------------------------------
# The reference's API over host bytes
# ---------------------------------------------------------------------------

def tsq_encode(data: bytes, ext: int, halo: bytes = b"") -> bytes:
    """tsqEncode (turbosqueeze.h:657): one block (<= 4 MiB) -> block stream.  Like the reference, the
    encoder looks a few bytes past the block (tsq_encode.cpp:74,126): `halo` is what follows the block
    in the caller's buffer (the next block's first bytes); zeros otherwise (canonical conditions)."""
    L = lib()
    n = len(data)
    src = C.create_string_buffer(bytes(data) + bytes(halo)[:128].ljust(128, b"\0"), n + 128)
    dst = C.create_string_buffer(OUTPUT_SZ)
    sz = C.c_uint32(0)
    ctx = L.tsqAllocateContext()
    try:
        L.tsqInit(ctx)
        L.tsqEncode(ctx, src, dst, C.byref(sz), n, int(ext))
    finally:
        L.tsqDeallocateContext(ctx)
    if sz.value == 0:
        raise TsqError(2, "tsqEncode produced no output (no device?)")
    return dst.raw[: sz.value]


def tsq_decode(stream: bytes, ext: int) -> bytes:
    """tsqDecode (turbosqueeze.h:670): block stream -> block; b'' when *outputSize == 0."""
    L = lib()
    src = C.create_string_buffer(bytes(stream), len(stream))
    dst = C.create_string_buffer(BLOCK_SZ + 256)
    sz = C.c_uint32(0)
    L.tsqDecode(src, dst, C.byref(sz), len(stream), int(ext))
    return dst.raw[: sz.value]


def _take_malloced(ptr: C.c_void_p, size: int) -> bytes:
    try:
        return C.string_at(ptr, size)
    finally:
        _libc.free(ptr)


def tsq_compress_mt(data: bytes, ext: bool, progress=None):
    """tsqAllocateContextCompression_MT + tsqCompress_MT (memory -> memory) + deallocate."""
    L = lib()
    ctx = L.tsqAllocateContextCompression_MT(False)
    if not ctx:
        raise TsqError(1, "tsqAllocateContextCompression_MT returned NULL")
    try:
        buf = C.create_string_buffer(bytes(data), len(data))
        out, sz = C.c_void_p(), C.c_size_t(0)
        ok = L.tsqCompress_MT(ctx, buf, len(data), False, C.byref(out), C.byref(sz), False, bool(ext), 0)
        if not ok:
            return None
        return _take_malloced(out, sz.value)
    finally:
        L.tsqDeallocateContextCompression_MT(ctx)


def tsq_decompress_mt(blob: bytes):
    L = lib()
    ctx = L.tsqAllocateContextDecompression_MT(False)
    if not ctx:
        raise TsqError(1, "tsqAllocateContextDecompression_MT returned NULL")
    try:
        buf = C.create_string_buffer(bytes(blob), len(blob))
        out, sz = C.c_void_p(), C.c_size_t(0)
        ok = L.tsqDecompress_MT(ctx, buf, len(blob), False, C.byref(out), C.byref(sz), False)
        if not ok:
            return None
        return _take_malloced(out, sz.value)
    finally:
        L.tsqDeallocateContextDecompression_MT(ctx)
