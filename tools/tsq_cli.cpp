// tsq_cli -- command-line front end over libturbosqueeze_amd.so, the counterpart of the reference's
// sample program (sample/main.cpp: `tsq c|d|b`), written against include/turbosqueeze.h only.
//
//   tsq_cli c <in> <out.tsq> [--no-ext]     compress a file   (tsqCompress_MT, file -> file)
//   tsq_cli d <in.tsq> <out>                decompress a file (tsqDecompress_MT, file -> file)
//   tsq_cli b [file|--synthetic BYTES] [--no-ext] [--reps N]
//                                           memory -> memory benchmark of the _MT API (host buffers, so
//                                           PCIe transfers are INSIDE the timed region), wall clock, MB = 1e6 B.
//   tsq_cli x <in.tsq> <offset> <length> <out>
//                                           range read: the container goes to the device, an index is built
//                                           (tsqa_index_create) and bytes [offset, offset + length) of its
//                                           uncompressed data are read (tsqa_decompress_ranges) into <out>.
//   tsq_cli r <in.tsq> [delim]              records: the container goes to the device and the record count and the longest
//                                           record for the delimiter byte (default 10, a newline) are printed
//                                           (tsqa_records with no tables: nothing is decoded into memory).
//   tsq_cli f <in.tsq> <needle>             find: the container goes to the device and the number of places at which the bytes
//                                           of <needle> (1 .. 16) occur, and the first place's offset, are printed (tsqa_find
//                                           with a table of one entry: nothing is decoded into memory).
//   tsq_cli k <in.tsq>                      checksum: the container goes to the device and the data's size and its CRC-32 are printed,
//                                           the value zlib.crc32 gives for the original file (tsqa_crc32: nothing is decoded
//                                           into memory).
// Unlike the reference's benchmark (clock() summed over threads, divided by 1e5) this reports
// wall-clock MB/s.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "turbosqueeze.h"

extern "C" void tsq_synth_text(uint8_t* out, size_t n, uint64_t seed, double s);

static double now_s()
{
    using namespace std::chrono;
    return duration<double>(steady_clock::now().time_since_epoch()).count();
}

static int usage()
{
    fprintf(stderr, "usage: tsq_cli c <in> <out> [--no-ext] | d <in> <out> | b [file | --synthetic BYTES] [--no-ext] [--reps N]\n"
                    "       tsq_cli bf <in> <workdir> [--no-ext] [--reps N]   (file -> file -> file with warm contexts)\n"
                    "       tsq_cli x <in.tsq> <offset> <length> <out>       (uncompressed bytes [offset, offset + length))\n"
                    "       tsq_cli r <in.tsq> [delim]                       (record count and longest record for a delimiter byte, default 10)\n"
                    "       tsq_cli f <in.tsq> <needle>                      (how often the needle's bytes, 1 .. 16, occur, and where first)\n"
                    "       tsq_cli k <in.tsq>                               (the data's size and its CRC-32, zlib's, in hex)\n");
    return 2;
}

// x: a range read straight from the container in device memory
static int range_read(const std::string& in, uint64_t offset, uint64_t length, const std::string& out_path)
{
    FILE* f = fopen(in.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", in.c_str()); return 1; }
    fseek(f, 0, SEEK_END); const long sz = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> blob(sz > 0 ? (size_t)sz : 0);
    const bool read_ok = fread(blob.data(), 1, blob.size(), f) == blob.size();
    fclose(f);
    if (!read_ok) { fprintf(stderr, "short read\n"); return 1; }
    tsqa_ctx* ctx = nullptr;
    if (tsqa_create(-1, &ctx) != TSQA_OK) { fprintf(stderr, "no usable MI355X (gfx950) device\n"); return 1; }
    void *d_in = nullptr, *d_out = nullptr;
    tsqa_index* idx = nullptr;
    std::vector<uint8_t> got(length);
    int rc = TSQA_OK;
    if (hipMalloc(&d_in, blob.size() ? blob.size() : 1) != hipSuccess || hipMalloc(&d_out, length ? length : 1) != hipSuccess ||
        hipMemcpy(d_in, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
        fprintf(stderr, "device memory: %s\n", hipGetErrorString(hipGetLastError()));
        rc = TSQA_ERR_HIP;
    }
    if (rc == TSQA_OK && (rc = tsqa_index_create(ctx, d_in, blob.size(), &idx)) == TSQA_OK) {
        const tsqa_range r = {offset, length, 0};
        rc = tsqa_decompress_ranges(ctx, idx, &r, 1, d_out, length, nullptr);
    }
    if (rc != TSQA_OK && rc != TSQA_ERR_HIP) fprintf(stderr, "range read failed (%d): %s\n", rc, tsqa_last_error(ctx));
    if (rc == TSQA_OK && length && hipMemcpy(got.data(), d_out, length, hipMemcpyDeviceToHost) != hipSuccess) rc = TSQA_ERR_HIP;
    tsqa_index_destroy(idx);
    (void)hipFree(d_in); (void)hipFree(d_out);
    tsqa_destroy(ctx);
    if (rc != TSQA_OK) return 1;
    FILE* o = fopen(out_path.c_str(), "wb");
    if (!o || fwrite(got.data(), 1, got.size(), o) != got.size()) { fprintf(stderr, "cannot write %s\n", out_path.c_str()); if (o) fclose(o); return 1; }
    fclose(o);
    return 0;
}

// r: the record count and the longest record of a container for a delimiter byte, measured on the device
static int count_records(const std::string& in, uint32_t delim)
{
    FILE* f = fopen(in.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", in.c_str()); return 1; }
    fseek(f, 0, SEEK_END); const long sz = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> blob(sz > 0 ? (size_t)sz : 0);
    const bool read_ok = fread(blob.data(), 1, blob.size(), f) == blob.size();
    fclose(f);
    if (!read_ok) { fprintf(stderr, "short read\n"); return 1; }
    tsqa_ctx* ctx = nullptr;
    if (tsqa_create(-1, &ctx) != TSQA_OK) { fprintf(stderr, "no usable MI355X (gfx950) device\n"); return 1; }
    void *d_in = nullptr, *d_words = nullptr;                  // d_words: item_first_record[2], need[2], status
    tsqa_index* idx = nullptr;
    uint64_t words[5] = {0, 0, 0, 0, 0};
    int rc = TSQA_OK;
    if (hipMalloc(&d_in, blob.size() ? blob.size() : 1) != hipSuccess || hipMalloc(&d_words, sizeof(words)) != hipSuccess ||
        hipMemcpy(d_in, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
        fprintf(stderr, "device memory: %s\n", hipGetErrorString(hipGetLastError()));
        rc = TSQA_ERR_HIP;
    }
    if (rc == TSQA_OK && (rc = tsqa_index_create(ctx, d_in, blob.size(), &idx)) == TSQA_OK) {
        uint64_t* const w = static_cast<uint64_t*>(d_words);
        rc = tsqa_records(ctx, idx, delim, 0, 0, nullptr, nullptr, nullptr, w, w + 2, reinterpret_cast<int32_t*>(w + 4), nullptr);
        if (rc == TSQA_ERR_OVERFLOW) rc = TSQA_OK;             // (a call without tables only measures: every record is "too many")
    }
    if (rc != TSQA_OK && rc != TSQA_ERR_HIP) fprintf(stderr, "records failed (%d): %s\n", rc, tsqa_last_error(ctx));
    if (rc == TSQA_OK && hipMemcpy(words, d_words, sizeof(words), hipMemcpyDeviceToHost) != hipSuccess) rc = TSQA_ERR_HIP;
    const uint64_t total = idx ? tsqa_index_total(idx) : 0;
    tsqa_index_destroy(idx);
    (void)hipFree(d_in); (void)hipFree(d_words);
    tsqa_destroy(ctx);
    if (rc != TSQA_OK) return 1;
    printf("{\"bytes\": %llu, \"delim\": %u, \"records\": %llu, \"longest_record\": %llu}\n", (unsigned long long)total, delim,
           (unsigned long long)words[2], (unsigned long long)words[3]);
    return 0;
}

// f: how often a byte string occurs in a container's data and where it occurs first, found on the device
static int find_needle(const std::string& in, const std::string& needle)
{
    FILE* f = fopen(in.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", in.c_str()); return 1; }
    fseek(f, 0, SEEK_END); const long sz = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> blob(sz > 0 ? (size_t)sz : 0);
    const bool read_ok = fread(blob.data(), 1, blob.size(), f) == blob.size();
    fclose(f);
    if (!read_ok) { fprintf(stderr, "short read\n"); return 1; }
    tsqa_ctx* ctx = nullptr;
    if (tsqa_create(-1, &ctx) != TSQA_OK) { fprintf(stderr, "no usable MI355X (gfx950) device\n"); return 1; }
    void *d_in = nullptr, *d_words = nullptr;                  // d_words: item_first_hit[2], need, the first hit's offset, status
    tsqa_index* idx = nullptr;
    uint64_t words[5] = {0, 0, 0, 0, 0};
    int rc = TSQA_OK;
    if (hipMalloc(&d_in, blob.size() ? blob.size() : 1) != hipSuccess || hipMalloc(&d_words, sizeof(words)) != hipSuccess ||
        hipMemset(d_words, 0, sizeof(words)) != hipSuccess || hipMemcpy(d_in, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
        fprintf(stderr, "device memory: %s\n", hipGetErrorString(hipGetLastError()));
        rc = TSQA_ERR_HIP;
    }
    if (rc == TSQA_OK && (rc = tsqa_index_create(ctx, d_in, blob.size(), &idx)) == TSQA_OK) {
        uint64_t* const w = static_cast<uint64_t*>(d_words);
        rc = tsqa_find(ctx, idx, needle.data(), (uint32_t)needle.size(), TSQA_FIND_FLAT, 1, nullptr, w + 3, w, w + 2, reinterpret_cast<int32_t*>(w + 4),
                       nullptr);
        if (rc == TSQA_ERR_OVERFLOW) rc = TSQA_OK;             // (a table of one entry: every hit but the first is "too many")
    }
    if (rc != TSQA_OK && rc != TSQA_ERR_HIP) fprintf(stderr, "find failed (%d): %s\n", rc, tsqa_last_error(ctx));
    if (rc == TSQA_OK && hipMemcpy(words, d_words, sizeof(words), hipMemcpyDeviceToHost) != hipSuccess) rc = TSQA_ERR_HIP;
    const uint64_t total = idx ? tsqa_index_total(idx) : 0;
    tsqa_index_destroy(idx);
    (void)hipFree(d_in); (void)hipFree(d_words);
    tsqa_destroy(ctx);
    if (rc != TSQA_OK) return 1;
    if (words[2] != 0) printf("{\"bytes\": %llu, \"needle_bytes\": %zu, \"hits\": %llu, \"first_hit\": %llu}\n", (unsigned long long)total, needle.size(),
                              (unsigned long long)words[2], (unsigned long long)words[3]);
    else printf("{\"bytes\": %llu, \"needle_bytes\": %zu, \"hits\": 0, \"first_hit\": null}\n", (unsigned long long)total, needle.size());
    return 0;
}

// k: zlib's CRC-32 of a container's data, made on the device
static int checksum(const std::string& in)
{
    FILE* f = fopen(in.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", in.c_str()); return 1; }
    fseek(f, 0, SEEK_END); const long sz = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> blob(sz > 0 ? (size_t)sz : 0);
    const bool read_ok = fread(blob.data(), 1, blob.size(), f) == blob.size();
    fclose(f);
    if (!read_ok) { fprintf(stderr, "short read\n"); return 1; }
    tsqa_ctx* ctx = nullptr;
    if (tsqa_create(-1, &ctx) != TSQA_OK) { fprintf(stderr, "no usable MI355X (gfx950) device\n"); return 1; }
    void *d_in = nullptr, *d_words = nullptr;                  // d_words: the item's CRC, its status, the whole data's CRC, the call's status
    tsqa_index* idx = nullptr;
    uint32_t words[4] = {0, 0, 0, 0};
    int rc = TSQA_OK;
    if (hipMalloc(&d_in, blob.size() ? blob.size() : 1) != hipSuccess || hipMalloc(&d_words, sizeof(words)) != hipSuccess ||
        hipMemset(d_words, 0, sizeof(words)) != hipSuccess || hipMemcpy(d_in, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
        fprintf(stderr, "device memory: %s\n", hipGetErrorString(hipGetLastError()));
        rc = TSQA_ERR_HIP;
    }
    if (rc == TSQA_OK && (rc = tsqa_index_create(ctx, d_in, blob.size(), &idx)) == TSQA_OK) {
        uint32_t* const w = static_cast<uint32_t*>(d_words);
        rc = tsqa_crc32(ctx, idx, 0, w, reinterpret_cast<int32_t*>(w + 1), nullptr, w + 2, reinterpret_cast<int32_t*>(w + 3), nullptr);
    }
    if (rc != TSQA_OK && rc != TSQA_ERR_HIP) fprintf(stderr, "checksum failed (%d): %s\n", rc, tsqa_last_error(ctx));
    if (rc == TSQA_OK && hipMemcpy(words, d_words, sizeof(words), hipMemcpyDeviceToHost) != hipSuccess) rc = TSQA_ERR_HIP;
    const uint64_t total = idx ? tsqa_index_total(idx) : 0;
    tsqa_index_destroy(idx);
    (void)hipFree(d_in); (void)hipFree(d_words);
    tsqa_destroy(ctx);
    if (rc != TSQA_OK) return 1;
    printf("{\"bytes\": %llu, \"crc32\": \"0x%x\"}\n", (unsigned long long)total, words[2]);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return usage();
    const std::string mode = argv[1];
    bool ext = true;
    int reps = 3;
    size_t synthetic = 0;
    std::vector<std::string> pos;
    for (int i = 2; i < argc; ++i) {
        if (!strcmp(argv[i], "--no-ext")) ext = false;
        else if (!strcmp(argv[i], "--reps") && i + 1 < argc) reps = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--synthetic") && i + 1 < argc) synthetic = strtoull(argv[++i], nullptr, 10);
        else pos.push_back(argv[i]);
    }
    if (mode == "c" || mode == "d") {
        if (pos.size() != 2) return usage();
        uint8_t* out_path = reinterpret_cast<uint8_t*>(const_cast<char*>(pos[1].c_str()));
        uint8_t* in_path = reinterpret_cast<uint8_t*>(const_cast<char*>(pos[0].c_str()));
        bool ok;
        const double t0 = now_s();
        if (mode == "c") {
            TSQCompressionContext_MT* ctx = tsqAllocateContextCompression_MT(false);
            if (!ctx) { fprintf(stderr, "no usable MI355X (gfx950) device\n"); return 1; }
            ok = tsqCompress_MT(ctx, in_path, 0, true, &out_path, nullptr, true, ext, 0);
            tsqDeallocateContextCompression_MT(ctx);
        } else {
            TSQDecompressionContext_MT* ctx = tsqAllocateContextDecompression_MT(false);
            if (!ctx) { fprintf(stderr, "no usable MI355X (gfx950) device\n"); return 1; }
            ok = tsqDecompress_MT(ctx, in_path, 0, true, &out_path, nullptr, true);
            tsqDeallocateContextDecompression_MT(ctx);
        }
        fprintf(stderr, "%s: %s in %.3f s\n", mode == "c" ? "compress" : "decompress", ok ? "ok" : "FAILED", now_s() - t0);
        return ok ? 0 : 1;
    }
    if (mode == "x") {
        if (pos.size() != 4) return usage();
        return range_read(pos[0], strtoull(pos[1].c_str(), nullptr, 10), strtoull(pos[2].c_str(), nullptr, 10), pos[3]);
    }
    if (mode == "r") {
        if (pos.size() != 1 && pos.size() != 2) return usage();
        const unsigned long delim = pos.size() == 2 ? strtoul(pos[1].c_str(), nullptr, 10) : 10ul;
        if (delim > 255ul) { fprintf(stderr, "delim is one byte value, 0..255\n"); return 2; }
        return count_records(pos[0], (uint32_t)delim);
    }
    if (mode == "f") {
        if (pos.size() != 2) return usage();
        if (pos[1].empty() || pos[1].size() > TSQA_FIND_MAX_NEEDLE) { fprintf(stderr, "the needle is 1 .. %u bytes\n", TSQA_FIND_MAX_NEEDLE); return 2; }
        return find_needle(pos[0], pos[1]);
    }
    if (mode == "k") {
        if (pos.size() != 1) return usage();
        return checksum(pos[0]);
    }
    if (mode == "bf") {
        // file -> .tsq file -> file through the _MT API's file modes with the contexts allocated once (as sample/main.cpp:71-95 keeps
        // context allocation out of its timing): rep 0 warms up (pinned staging, HBM scratch, kernel load), the best of the others counts
        if (pos.size() != 2) return usage();
        const std::string packed = pos[1] + "/bf.tsq", back = pos[1] + "/bf.out";
        uint8_t* in_path = reinterpret_cast<uint8_t*>(const_cast<char*>(pos[0].c_str()));
        uint8_t* packed_path = reinterpret_cast<uint8_t*>(const_cast<char*>(packed.c_str()));
        uint8_t* back_path = reinterpret_cast<uint8_t*>(const_cast<char*>(back.c_str()));
        TSQCompressionContext_MT* cctx = tsqAllocateContextCompression_MT(false);
        TSQDecompressionContext_MT* dctx = tsqAllocateContextDecompression_MT(false);
        if (!cctx || !dctx) { fprintf(stderr, "no usable MI355X (gfx950) device\n"); return 1; }
        double best_c = 1e30, best_d = 1e30;
        for (int r = 0; r <= reps; ++r) {
            remove(packed.c_str()); remove(back.c_str());
            const double t0 = now_s();
            if (!tsqCompress_MT(cctx, in_path, 0, true, &packed_path, nullptr, true, ext, 0)) { fprintf(stderr, "compress failed\n"); return 1; }
            const double t1 = now_s();
            if (!tsqDecompress_MT(dctx, packed_path, 0, true, &back_path, nullptr, true)) { fprintf(stderr, "decompress failed\n"); return 1; }
            const double t2 = now_s();
            if (r > 0) { if (t1 - t0 < best_c) best_c = t1 - t0; if (t2 - t1 < best_d) best_d = t2 - t1; }
        }
        tsqDeallocateContextCompression_MT(cctx);
        tsqDeallocateContextDecompression_MT(dctx);
        auto fsize = [](const std::string& p) -> size_t { FILE* f = fopen(p.c_str(), "rb"); if (!f) return 0; fseek(f, 0, SEEK_END); long n = ftell(f); fclose(f); return n < 0 ? 0 : (size_t)n; };
        const size_t n = fsize(pos[0]), c = fsize(packed);
        // byte-for-byte comparison of the round trip, 64 MiB at a time
        bool exact = n == fsize(back);
        if (exact) {
            FILE* a = fopen(pos[0].c_str(), "rb"); FILE* b = fopen(back.c_str(), "rb");
            std::vector<uint8_t> x(size_t(64) << 20), y(size_t(64) << 20);
            for (size_t got; exact && (got = fread(x.data(), 1, x.size(), a)) > 0;) exact = fread(y.data(), 1, got, b) == got && memcmp(x.data(), y.data(), got) == 0;
            fclose(a); fclose(b);
        }
        printf("{\"mode\": \"file to file\", \"input_bytes\": %zu, \"compressed_bytes\": %zu, \"ext\": %d, \"output_correct\": %s, "
               "\"compress_GBps_wall\": %.2f, \"decompress_GBps_wall\": %.2f, \"compress_s\": %.3f, \"decompress_s\": %.3f, \"reps\": %d}\n",
               n, c, ext ? 1 : 0, exact ? "true" : "false", (double)n / best_c / 1e9, (double)n / best_d / 1e9, best_c, best_d, reps);
        return exact ? 0 : 1;
    }
    if (mode != "b") return usage();

    std::vector<uint8_t> input;
    if (!pos.empty()) {
        FILE* f = fopen(pos[0].c_str(), "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", pos[0].c_str()); return 1; }
        fseek(f, 0, SEEK_END); long sz = ftell(f); fseek(f, 0, SEEK_SET);
        input.resize((size_t)sz);
        if (fread(input.data(), 1, input.size(), f) != input.size()) { fprintf(stderr, "short read\n"); return 1; }
        fclose(f);
    } else {
        input.resize(synthetic ? synthetic : (size_t)1000000000);
        tsq_synth_text(input.data(), input.size(), 1, 0.0);           // enwik9-shaped text
    }
    TSQCompressionContext_MT* cctx = tsqAllocateContextCompression_MT(false);
    TSQDecompressionContext_MT* dctx = tsqAllocateContextDecompression_MT(false);
    if (!cctx || !dctx) { fprintf(stderr, "no usable MI355X (gfx950) device\n"); return 1; }
    double best_c = 1e30, best_d = 1e30;
    size_t csize = 0;
    bool exact = true;
    for (int r = 0; r <= reps; ++r) {                                  // r == 0 warms up (pinned buffers, HBM scratch)
        uint8_t* comp = nullptr; size_t comp_sz = 0;
        double t0 = now_s();
        if (!tsqCompress_MT(cctx, input.data(), input.size(), false, &comp, &comp_sz, false, ext, 0)) { fprintf(stderr, "compress failed\n"); return 1; }
        double t1 = now_s();
        uint8_t* back = nullptr; size_t back_sz = 0;
        if (!tsqDecompress_MT(dctx, comp, comp_sz, false, &back, &back_sz, false)) { fprintf(stderr, "decompress failed\n"); return 1; }
        double t2 = now_s();
        exact = exact && back_sz == input.size() && memcmp(back, input.data(), back_sz) == 0;
        csize = comp_sz;
        free(comp); free(back);
        if (r > 0) { if (t1 - t0 < best_c) best_c = t1 - t0; if (t2 - t1 < best_d) best_d = t2 - t1; }
    }
    tsqDeallocateContextCompression_MT(cctx);
    tsqDeallocateContextDecompression_MT(dctx);
    printf("{\"input_bytes\": %zu, \"compressed_bytes\": %zu, \"ratio\": %.4f, \"ext\": %d, \"output_correct\": %s, "
           "\"compress_MBps_wall_host_buffers\": %.1f, \"decompress_MBps_wall_host_buffers\": %.1f, \"reps\": %d}\n",
           input.size(), csize, (double)csize / (double)input.size(), ext ? 1 : 0, exact ? "true" : "false",
           (double)input.size() / best_c / 1e6, (double)input.size() / best_d / 1e6, reps);
    return exact ? 0 : 1;
}
