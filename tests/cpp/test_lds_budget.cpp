// The LDS sums of a workgroup (search_kernels.hpp: pure host functions) against numbers worked out by hand from the formulas of the
// driver as it stood before the functions existed, the clamp as a function of an assumed limit, and the refusal's message.
// Host only: built by tests/test_lds_budget.py with the C++ compiler, no device needed.
#include <cstdio>
#include <cstdlib>
#include <string>
#include "search_kernels.hpp"

using namespace hnswgpu;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static uint32_t ceil_log2(uint64_t v) {
    uint32_t b = 0;
    while ((1ull << b) < v) ++b;
    return b;
}

// a strict one-query launch as SearchCall::plan and shape_launch size it: (bytes with 256 entries of the literal heap, table bits)
struct Launch {
    size_t lds256, lds512, lean;
    uint32_t tb;
    int table;
    bool clamped;
};
static Launch launch(int metric, uint32_t d, uint64_t n, uint64_t ef, uint32_t deg_stride, size_t limit, uint32_t force_tbits = 0) {
    const uint32_t tile = tile_bytes_for(metric, (d + 31) / 32 * 32);
    int slots = 1;
    while ((uint64_t)slots * 64 < ef) slots *= 2;
    if (slots == 8) slots = 16;
    if (deg_stride > 64) slots = 16;
    const uint32_t idbits = ceil_log2(n) ? ceil_log2(n) : 1;
    uint32_t tbits = ceil_log2(ef * (deg_stride < 64 ? deg_stride : 64));
    tbits = tbits < 8 ? 8 : tbits > 14 ? 14 : tbits;
    if (force_tbits) tbits = force_tbits;
    const uint32_t me = merge_entries_for(slots, true);
    const VisitedTable t = fit_visited_table(tile, tbits, idbits, ((size_t)me + CAND_LDS_MIN) * sizeof(hent_t), limit);
    const VisitedTable tl = fit_visited_table(tile, tbits, idbits, (size_t)merge_entries_for(slots, false) * sizeof(hent_t), limit);
    return Launch{search_lds_bytes(tile, t.bytes, me, 256), search_lds_bytes(tile, t.bytes, me, 512),
                  search_lds_bytes(tile, tl.bytes, merge_entries_for(slots, false), 0), t.tb, t.table, t.clamped};
}

int main() {
    const size_t KIB64 = 65536, KIB160 = 163840;
    // ---- the table of the issue: S = 4, tb = 14, 16-bit cells, strict: tile + 256 + 32768 + 2560 + 2048 (or 4096)
    {
        const Launch a = launch(DIST_L2, 4096, 60000, 200, 64, KIB160);
        CHECK(a.lds256 == 54016 && a.lds512 == 56064 && a.tb == 14 && a.table == TABLE_LDS_CELL16 && !a.clamped);
        const Launch b = launch(DIST_L2, 8000, 60000, 200, 64, KIB160);
        CHECK(b.lds256 == 69632 && b.lds512 == 71680 && b.tb == 14 && !b.clamped);
        const Launch c = launch(DIST_L2, 128, 60000, 200, 64, KIB160);
        CHECK(c.lds256 == 512 + 256 + 32768 + 2560 + 2048 && c.lds256 == 38144);   // "about 38 000"
    }
    // ---- the six configurations of bench.py: exactly the bytes the driver added up before (worked out by hand from its formulas)
    {
        const Launch sift = launch(DIST_L2, 128, 1000000, 64, 32, KIB64);             // 512 + 256 + 2 << 11 + 128 x 8 + heap
        CHECK(sift.lds256 == 7936 && sift.lds512 == 9984 && sift.lean == 5888 && sift.tb == 11 && sift.table == TABLE_LDS_CELL16);
        const Launch glove = launch(DIST_COSINE, 25, 1200000, 128, 48, KIB64);        // 144 + 256 + 2 << 13 + 192 x 8 + heap
        CHECK(glove.lds256 == 20368 && glove.lds512 == 22416 && glove.tb == 13 && glove.table == TABLE_LDS_CELL16);
        const Launch dot = launch(DIST_DOT, 25, 1200000, 128, 48, KIB64);
        CHECK(dot.lds256 == 20352 && dot.lds512 == 22400 && dot.tb == 13);
        const Launch mnist = launch(DIST_L2, 784, 60000, 200, 64, KIB64);             // 3200 + 256 + 2 << 14 + 320 x 8 + heap
        CHECK(mnist.lds256 == 40832 && mnist.lds512 == 42880 && mnist.tb == 14 && mnist.table == TABLE_LDS_CELL16);
        const Launch hbm = launch(DIST_L2, 784, 240000, 200, 64, KIB64);
        CHECK(hbm.lds256 == 40832 && hbm.lds512 == 42880 && hbm.tb == 14);
        const Launch rnd = launch(DIST_L2, 25, 10000, 24, 32, KIB64);                 // 128 + 256 + 2 << 10 + 128 x 8 + heap
        CHECK(rnd.lds256 == 5504 && rnd.lds512 == 7552 && rnd.tb == 10);
        for (const Launch& l : {sift, glove, dot, mnist, hbm, rnd}) CHECK(!l.clamped);
        // 17 id bits and a table of 2^6 cells: 14 bits do not fit a 16-bit cell
        const VisitedTable c32 = visited_table_for(6, 17);
        CHECK(c32.table == TABLE_LDS_CELL32 && c32.tb == 6 && c32.bytes == 256);
        const VisitedTable small = visited_table_for(14, 9);                          // 300 points: at most 2^12 cells
        CHECK(small.tb == 12 && small.table == TABLE_LDS_CELL16 && small.restbits == 0 && small.bytes == 8192);
    }
    // ---- the clamp, as a function of the limit
    {
        // d = 8000 at 64 KiB: 69 632 does not fit; tb 13 (53 248 bytes) does, and leaves room for 512 heap entries
        const Launch a = launch(DIST_L2, 8000, 60000, 200, 64, KIB64);
        CHECK(a.clamped && a.tb == 13 && a.table == TABLE_LDS_CELL16 && a.lds256 == 53248 && a.lds512 == 55296 && a.lds512 <= KIB64);
        // ... and at 160 KiB nothing is clamped
        CHECK(!launch(DIST_L2, 8000, 60000, 200, 64, KIB160).clamped);
        // d = 4096 fits 64 KiB as it is
        CHECK(!launch(DIST_L2, 4096, 60000, 200, 64, KIB64).clamped);
        // 2^20 points and 1536 bytes of room for the table: 16-bit cells hold 13 id bits, so below tb = 10 the cells are 32 bits wide
        // and the step from 10 to 9 frees nothing (2 << 10 == 4 << 9); 2^8 cells of 32 bits fit
        const uint32_t tile = tile_bytes_for(DIST_L2, 14784);
        const VisitedTable t = fit_visited_table(tile, 14, 20, 4608, KIB64);
        CHECK(tile == 59136 && t.clamped && t.tb == 8 && t.table == TABLE_LDS_CELL32 && t.bytes == 1024 &&
              search_lds_bytes(tile, t.bytes, 320, 256) == 59136 + 256 + 1024 + 4608);
        CHECK(visited_table_for(10, 20).table == TABLE_LDS_CELL16 && visited_table_for(9, 20).table == TABLE_LDS_CELL32);
        CHECK(search_lds_bytes(tile, visited_table_for(10, 20).bytes, 320, 256) > KIB64 && search_lds_bytes(tile, visited_table_for(9, 20).bytes, 320, 256) > KIB64);
        // the smallest stride at which 2^14 cells no longer fit beside 256 heap entries: tile + 256 + 32768 + 2560 + 2048 > limit
        for (size_t limit : {KIB64, KIB160}) {
            const uint32_t rs_fit = (uint32_t)((limit - 256 - 32768 - 4608) / 4 / 32 * 32);
            CHECK(!fit_visited_table(4 * rs_fit, 14, 16, 4608, limit).clamped);
            CHECK(fit_visited_table(4 * (rs_fit + 32), 14, 16, 4608, limit).clamped && fit_visited_table(4 * (rs_fit + 32), 14, 16, 4608, limit).tb == 13);
            CHECK(rs_fit == (limit == KIB64 ? 6976u : 31552u));
        }
        // a lean launch keeps nothing behind the table with 16 slots
        CHECK(merge_entries_for(16, true) == 0 && merge_entries_for(4, true) == 320 && merge_entries_for(4, false) == 0 && merge_entries_for(2, false) == 192);
    }
    // ---- the other launches
    {
        CHECK(descend_lds_bytes(16384, false) == 16640 && descend_lds_bytes(16384, true) == 33024);
        CHECK(descend_lds_bytes(32000, true) == 64256 && descend_lds_bytes(32768, true) > KIB64);
        // the literal-heap kernel: 10 KiB where tile + ids leave more than 4 KiB of it, else tile + ids + 4 KiB
        const ExactLds a = exact_lds(512, 1100, 1000000);                 // d = 128: 9472 bytes of heaps
        CHECK(a.lds == 10240 && a.r_lds_cap == 592 && a.cand_lds == 592);
        const ExactLds b = exact_lds(4096, 100, 64);                      // d = 1024: 5888 bytes, return_points whole, the cap decides
        CHECK(b.r_lds_cap == 102 && b.cand_lds == 64 && b.lds == 4352 + 166 * 8);
        CHECK(exact_lds(4096, 100, 1200).cand_lds == 634);
        const ExactLds c = exact_lds(8192, 100, 1200);                    // d = 2048: the floor of 4096 bytes
        CHECK(c.r_lds_cap == 102 && c.cand_lds == 410 && c.lds == 8192 + 256 + 4096);
        const ExactLds e = exact_lds(16384, 1100, 1000);                  // d = 4096, ef = 1100: return_points no longer fits
        CHECK(e.r_lds_cap == 256 && e.cand_lds == 256 && e.lds == 16384 + 256 + 4096);
        CHECK(build_search_lds_bytes(4096, 12) == 4096 + 256 + 8192 && build_select_lds_bytes(4096, 24) == 4096 + 256 + 192);
        CHECK(pair_lds_bytes(4240, 12, 100) == 27392);                    // (DistCosine d = 1054 at ef = 100, 2^12 cells)
    }
    // ---- the refusal
    {
        CHECK(min_workgroup_lds_bytes(1000) == 1000 + 256 + 32 + 2560 + 2048);
        CHECK(lds_refusal(8000, 32000, KIB64).empty() && lds_refusal(8000, 32000, KIB160).empty());
        // the smallest stride whose tile does not fit: 4 rs + 4896 > limit
        CHECK(lds_refusal(15136, 4 * 15136, KIB64).empty() && !lds_refusal(15137, 4 * 15168, KIB64).empty());
        CHECK(lds_refusal(39712, 4 * 39712, KIB160).empty() && !lds_refusal(39713, 4 * 39744, KIB160).empty());
        std::printf("message: %s\n", lds_refusal(39713, 4 * 39744, KIB160).c_str());
    }
    if (failures) return 1;
    std::printf("lds budget OK\n");
    return 0;
}
