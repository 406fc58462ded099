"""turbosqueeze_amd -- MI355X (gfx950) implementation of turbosqueeze's per-block
encode/decode hot path.  This Python package is a thin ctypes face over
libturbosqueeze_amd.so (hand-written HIP kernels behind the C ABI of
include/turbosqueeze_amd.h); it holds no codec logic and has no CPU fallback:
if the shared library or a gfx950 device is missing, calls raise.
"""
from .api import (  # noqa: F401
    BLOCK_SZ,
    OUTPUT_SZ,
    BatchIndex,
    BatchItem,
    BlockGroup,
    DeviceBatchIndex,
    DeviceCodec,
    ItemRange,
    PackedBatch,
    Range,
    RangeIndex,
    RangeItem,
    SizedIndex,
    TsqError,
    batch_bound,
    build_info,
    build_native,
    container_bound,
    lib,
    lib_path,
    plan_batch,
    plan_batch_split,
    plan_compress_tables,
    plan_compress_tables_split,
    plan_cut,
    plan_cut_items,
    plan_gather,
    plan_gather_rows,
    plan_index_packed,
    plan_dense,
    plan_item_ranges,
    plan_join,
    plan_packed,
    plan_ranges,
    plan_split,
    source_fingerprint,
    tsq_compress_mt,
    tsq_decode,
    tsq_decompress_mt,
    tsq_encode,
)
from . import synth  # noqa: F401
