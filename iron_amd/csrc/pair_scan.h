// Multi-level exclusive prefix scan over pairs of int64 (pair_scan.hip), shared by marching cubes (vertex and triangle counts per
// block) and the texture bake (samples per face, faces with a sample).  Level 0 holds the caller's entries; every level is scanned
// in place, 1024 entries per block, with the block totals written one level up, until one entry is left; the higher-level offsets
// are then added back down.  After pair_scan level 0 holds the exclusive prefixes and the top level the one total.  Integer sums
// in a fixed structure: bitwise deterministic.
#pragma once
#include "host_util.h"

namespace iron {

constexpr int kScanBlock = 1024;

struct Pair64 {
    int64_t a, b;
};

struct ScanLevels {
    int levels;            // scan levels; level `levels` holds the one total entry
    int64_t level_len[24];
    size_t level_off[25];  // byte offsets of the Pair64 arrays, each 256-byte aligned
    Pair64* level(void* ws, int l) const { return ws_ptr<Pair64>(ws, level_off[l]); }
    const Pair64* level(const void* ws, int l) const { return ws_ptr<Pair64>(ws, level_off[l]); }
};

// the levels of a scan over n entries, carved at the running offset of a workspace layout
inline ScanLevels scan_levels(int64_t n, Carver& c) {
    ScanLevels S{};
    int lv = 0;
    for (int64_t len = n;; len = (len + kScanBlock - 1) / kScanBlock, ++lv) {
        S.level_len[lv] = len;
        S.level_off[lv] = c.take(sizeof(Pair64) * (size_t)len);
        if (lv > 0 && len == 1) break;
    }
    S.levels = lv;
    return S;
}

// up sweep and down sweep on `st`; IRON_OK or IRON_ERR_HIP
int pair_scan(const ScanLevels& S, void* ws, hipStream_t st);

}  // namespace iron
