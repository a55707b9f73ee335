// ScratchLayout (csrc/scratch_layout.hpp: plain arithmetic, no HIP) over host blocks: the size and the carving agree, every array
// starts on a 256-byte boundary and none overlaps another, a span between two marks is what lies between them, counts of 0, of 1
// and of whole multiples of 256 bytes, a list that grew after the block was sized is refused, the uploads of a host form with two
// arrays absent (Uploads: the pointers turn from host to block addresses, an absent one stays null), and three blocks of the host
// units against the byte counts those units summed by hand before the layout existed.
// Host only: built by tests/test_scratch_layout.py with g++ -fsanitize=address,undefined, no device needed.  Every array is
// written over its whole length, so an array that reached past its block would stop the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scratch_layout.hpp"

using namespace hnswgpu;

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

// a block of exactly `bytes` (one at least) on a 256-byte boundary
struct Block {
    unsigned char* p;
    uint64_t bytes;
    explicit Block(uint64_t n) : p(static_cast<unsigned char*>(std::aligned_alloc(256, (size_t)round_up(n ? n : 1, 256)))), bytes(n) {}
    ~Block() { std::free(p); }
};

struct Extent {
    const void* at;
    uint64_t bytes;  // what the array's owner writes: count * sizeof(T)
};
// inside the block, aligned, in order, not overlapping; and every byte of every array can be written
static void check_extents(const Block& b, const std::vector<Extent>& arrays) {
    const unsigned char* end_of_last = b.p;
    for (const Extent& e : arrays) {
        const unsigned char* at = static_cast<const unsigned char*>(e.at);
        CHECK(at != nullptr && (reinterpret_cast<uintptr_t>(at) & 255u) == 0);
        CHECK(at >= end_of_last && at + e.bytes <= b.p + b.bytes);
        std::memset(const_cast<unsigned char*>(at), 0x5A, (size_t)e.bytes);
        end_of_last = at + e.bytes;
    }
}

// dendrogram.hip, dendrogram_of_edges: la, lb (m words each), parent, top, wsum, w (n + m words each), the word
static void dendrogram_block(uint64_t n, uint64_t m) {
    const uint64_t labels = n + m;
    uint32_t *la, *lb, *parent, *top, *wsum, *w, *word;
    ScratchLayout lay;
    lay.arrays(m, la, lb);
    lay.arrays(labels, parent, top, wsum, w);
    lay.array(word, 64);
    const uint64_t bm = round_up(m * 4, 256), bl = round_up(labels * 4, 256);
    CHECK(lay.size() == 2 * bm + 4 * bl + 256);
    Block b(lay.size());
    CHECK(lay.place(b.p, b.bytes));
    check_extents(b, {{la, m * 4}, {lb, m * 4}, {parent, labels * 4}, {top, labels * 4}, {wsum, labels * 4}, {w, labels * 4}, {word, 256}});
    CHECK(reinterpret_cast<unsigned char*>(word) == b.p + 2 * bm + 4 * bl);
}

// graph_components.hip, forest_init: parent, mark, number_of (n + 1 words each)
static void forest_block(uint64_t n) {
    uint32_t *parent, *mark, *number_of;
    ScratchLayout lay;
    lay.array(parent, n + 1);
    lay.array(mark, n + 1);
    lay.array(number_of, n + 1);
    CHECK(lay.size() == 3 * round_up((n + 1) * 4, 256));
    Block b(lay.size());
    CHECK(lay.place(b.p, b.bytes));
    check_extents(b, {{parent, (n + 1) * 4}, {mark, (n + 1) * 4}, {number_of, (n + 1) * 4}});
}

// symmetric_graph.hip, stage_directed_graph: the StagedGraph of n rows of k slots -- ids, dists, rank (n k each), counts (n), layer
static void staged_graph_block(uint64_t n, uint64_t k) {
    const uint64_t slots = n * k;
    uint64_t* ids;
    float* dists;
    int32_t* rank;
    uint32_t* counts;
    uint8_t* layer;
    ScratchLayout lay;
    lay.arrays(slots, ids, dists, rank);  // (of three element sizes: each padded on its own)
    lay.array(counts, n);
    lay.array(layer, slots);
    CHECK(lay.size() == round_up(slots * 8, 256) + 2 * round_up(slots * 4, 256) + round_up(n * 4, 256) + round_up(slots, 256));
    CHECK(lay.size() >= 17 * n * k + 4 * n && lay.size() < 17 * n * k + 4 * n + 5 * 256);  // "17 n k + 4 n bytes (and padding)"
    Block b(lay.size());
    CHECK(lay.place(b.p, b.bytes));
    check_extents(b, {{ids, slots * 8}, {dists, slots * 4}, {rank, slots * 4}, {counts, n * 4}, {layer, slots}});
}

int main() {
    // ---- counts of 0, of 1, of exactly 256 bytes; the size is what the carving uses
    {
        uint32_t *none, *one, *line, *two_lines;
        uint8_t* byte;
        double* last;
        ScratchLayout lay;
        CHECK(lay.size() == 0);
        lay.array(none, 0);
        CHECK(lay.size() == 0);
        lay.array(one, 1);
        CHECK(lay.size() == 256);
        lay.array(line, 64);  // 256 bytes as they are: no padding added
        CHECK(lay.size() == 512);
        lay.array(two_lines, 65);
        CHECK(lay.size() == 1024);
        lay.array(byte, 1);
        lay.array(last, 32);  // 256 bytes again
        CHECK(lay.size() == 1536);
        Block b(lay.size());
        CHECK(lay.place(b.p, b.bytes));
        CHECK(reinterpret_cast<unsigned char*>(none) == b.p && reinterpret_cast<unsigned char*>(one) == b.p);  // (an empty array owns nothing)
        CHECK(reinterpret_cast<unsigned char*>(line) == b.p + 256 && reinterpret_cast<unsigned char*>(two_lines) == b.p + 512);
        CHECK(byte == b.p + 1024 && reinterpret_cast<unsigned char*>(last) == b.p + 1280);
        check_extents(b, {{one, 4}, {line, 256}, {two_lines, 260}, {byte, 1}, {last, 256}});
    }
    // ---- bytes() takes what it is told, skip() belongs to nobody: a block may end unpadded or with a line of its own
    {
        uint32_t *label, *sizes;
        ScratchLayout lay;
        lay.array(label, 100);
        lay.bytes(sizes, 7 * 4);
        CHECK(lay.size() == 512 + 28);
        lay.skip(256);
        CHECK(lay.size() == 512 + 28 + 256);
        Block b(lay.size());
        CHECK(lay.place(b.p, b.bytes));
        CHECK(reinterpret_cast<unsigned char*>(sizes) == b.p + 512);
        check_extents(b, {{label, 400}, {sizes, 28}});
    }
    // ---- a span between two marks: the arrays named between them, padding included
    {
        uint32_t *before, *first, *second, *after;
        unsigned long long* third;
        ScratchLayout lay;
        lay.array(before, 3);
        const uint64_t from = lay.size();
        lay.array(first, 100);
        lay.array(second, 100);
        lay.array(third, 100);
        const uint64_t span = lay.size() - from;
        lay.array(after, 5);
        CHECK(from == 256 && span == 512 + 512 + 1024);
        Block b(lay.size());
        CHECK(lay.place(b.p, b.bytes));
        CHECK(reinterpret_cast<unsigned char*>(first) == b.p + from);
        CHECK(reinterpret_cast<unsigned char*>(first) + span == reinterpret_cast<unsigned char*>(after));
        CHECK(reinterpret_cast<unsigned char*>(third) + round_up(100 * 8, 256) == reinterpret_cast<unsigned char*>(first) + span);
        std::memset(first, 0, (size_t)span);  // what a caller does with a span
        check_extents(b, {{before, 12}, {first, 400}, {second, 400}, {third, 800}, {after, 20}});
    }
    // ---- a list that changed after the block was sized is reported, and nothing is carved
    {
        uint32_t *a = nullptr, *late = nullptr;
        uint32_t sentinel = 0;
        ScratchLayout lay;
        lay.array(a, 10);
        Block b(lay.size());
        lay.array(late, 10);  // named after the sizing
        a = &sentinel;
        CHECK(!lay.place(b.p, b.bytes));
        CHECK(a == &sentinel && late == nullptr);
        // no block at all
        ScratchLayout other;
        other.array(a, 10);
        CHECK(!other.place(nullptr, other.size()) && a == &sentinel);
        // more arrays than a layout holds: refused as a whole
        uint32_t* many[ScratchLayout::MAX_ARRAYS + 1] = {};
        ScratchLayout full;
        for (uint32_t*& p : many) full.array(p, 1);
        Block big((uint64_t)(ScratchLayout::MAX_ARRAYS + 1) * 256);
        CHECK(!full.place(big.p, big.bytes) && many[0] == nullptr);
        // a block larger than the layout (a pool's block reused) is fine
        ScratchLayout small;
        small.array(a, 10);
        CHECK(small.place(big.p, big.bytes) && reinterpret_cast<unsigned char*>(a) == big.p);
    }
    // ---- Uploads: a host form's arrays named into the block; two of the five are absent, one is there with no element
    {
        const uint32_t host_parent[5] = {0xFFFFFFFFu, 0, 0, 1, 1};
        const float host_core[70] = {};
        const uint8_t host_selected[5] = {0, 1, 1, 0, 0};
        const uint32_t *parent = host_parent, *point_cluster = nullptr, *empty = host_parent;
        const float* core = host_core;
        const uint8_t* selected = host_selected;
        const double* death = nullptr;
        uint32_t* scratch;
        ScratchLayout lay;
        Uploads ups;
        lay.array(scratch, 10);
        ups.brings(lay, 5, parent, point_cluster);  // (point_cluster: absent)
        ups.bring(lay, core, 70);
        ups.brings(lay, 5, selected, death);  // (death: absent)
        ups.bring(lay, empty, 0);
        CHECK(ups.count() == 4 && lay.size() == 256 + 256 + 512 + 256);
        CHECK(parent == host_parent && core == host_core);  // (nothing moves before the block is there)
        Block b(lay.size());
        CHECK(lay.place(b.p, b.bytes));
        CHECK(point_cluster == nullptr && death == nullptr);
        CHECK(reinterpret_cast<const unsigned char*>(parent) == b.p + 256 && reinterpret_cast<const unsigned char*>(core) == b.p + 512);
        CHECK(selected == b.p + 1024 && reinterpret_cast<const unsigned char*>(empty) == b.p + 1280);
        check_extents(b, {{scratch, 40}, {parent, 20}, {core, 280}, {selected, 5}});
        const struct { const void* to; const void* from; uint64_t bytes; } want[] = {
            {parent, host_parent, 20}, {core, host_core, 280}, {selected, host_selected, 5}, {empty, host_parent, 0}};
        for (int i = 0; i < ups.count(); ++i) {
            void* to;
            const void* from;
            uint64_t bytes;
            ups.item(i, to, from, bytes);
            CHECK(to == want[i].to && from == want[i].from && bytes == want[i].bytes);
            std::memcpy(to, from, (size_t)bytes);  // what copy_uploads asks of the runtime
        }
        CHECK(parent[0] == 0xFFFFFFFFu && parent[4] == 1 && selected[1] == 1 && selected[4] == 0);
    }
    // ---- three blocks of the host units against the sums written by hand before
    for (uint64_t n : {1, 2, 63, 64, 65, 1000}) {
        forest_block(n);
        for (uint64_t m : {1, 2, 63, 64, 65, 1000}) dendrogram_block(n, m);
        for (uint64_t k : {1, 2, 63, 64, 65, 1000}) staged_graph_block(n, k);
    }
    if (failures) return 1;
    std::printf("scratch layout OK\n");
    return 0;
}
