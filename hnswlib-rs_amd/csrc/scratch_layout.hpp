// scratch_layout.hpp -- the one place where a block of scratch memory is divided into arrays: the host units name their arrays
// once, the layout says how many bytes the block needs and, once the block is there, hands every array its pointer.  A byte count
// and a carving that disagree cannot be written down.  Uploads, below it, names the arrays that a host form brings along into the
// same block.  Plain arithmetic, no HIP: hip_host.hpp includes it for the .hip units, and
// tests/cpp/test_scratch_layout.cpp compiles it on its own.  Private: not installed, not part of the ABI.
#pragma once
#include <cstdint>
#include <cstring>

namespace hnswgpu {

inline uint64_t round_up(uint64_t x, uint64_t m) { return (x + m - 1) / m * m; }

// Usage: name the arrays in their order in the block (array / arrays / bytes / skip), allocate size() bytes, place() the block.  The
// pointers named must live until place() returns; it writes all of them or none.
class ScratchLayout {
public:
    static constexpr uint64_t ALIGN = 256;  // every array starts on such a boundary and is padded to one
    static constexpr int MAX_ARRAYS = 48;

    // `count` T behind what was named before, padded to ALIGN bytes
    template <typename T>
    void array(T*& out, uint64_t count) { bytes(out, round_up(count * sizeof(T), ALIGN)); }
    // arrays of `count` elements each, one behind the other
    template <typename... Ts>
    void arrays(uint64_t count, Ts*&... outs) { (array(outs, count), ...); }
    // exactly `n` bytes: a region whose size the caller has padded itself, or the last one of a block that ends unpadded
    template <typename T>
    void bytes(T*& out, uint64_t n) {
        if (used_ == MAX_ARRAYS) { broken_ = true; return; }
        slot_[used_++] = Slot{&out, total_};
        total_ += n;
    }
    // `n` bytes that belong to nobody
    void skip(uint64_t n) { total_ += n; }

    // the bytes named so far: the block's size at the end, a mark in between (the span between two marks: their difference)
    uint64_t size() const { return total_; }

    // The block is at `base` and holds `capacity` bytes.  False, and no pointer written, when the arrays named do not fit: more
    // were named after the block was sized, or more than MAX_ARRAYS.
    bool place(void* base, uint64_t capacity) {
        if (broken_ || base == nullptr || total_ > capacity) return false;
        for (int i = 0; i < used_; ++i) {
            unsigned char* at = static_cast<unsigned char*>(base) + slot_[i].offset;
            std::memcpy(slot_[i].out, &at, sizeof(at));  // (every T* is an object pointer: one representation)
        }
        return true;
    }

private:
    struct Slot {
        void* out;  // a T*& of the caller's
        uint64_t offset;
    };
    Slot slot_[MAX_ARRAYS];
    int used_ = 0;
    bool broken_ = false;
    uint64_t total_ = 0;
};

// The host arrays that a host form brings to the device inside its block.  bring() takes a pointer that holds the HOST address: it
// notes that address and names the pointer into the layout, so place() replaces it by the address of the device copy; an absent
// array (nullptr) names nothing and stays null.  Once the block is placed, item() says what to copy where (hip_host.hpp:
// copy_uploads).  The pointers must live as long as the list.
class Uploads {
public:
    template <typename T>
    void bring(ScratchLayout& lay, const T*& p, uint64_t count) {
        if (p == nullptr) return;
        // (a full list: the layout, which holds as many, is full too and refuses the block)
        if (used_ < ScratchLayout::MAX_ARRAYS) item_[used_++] = Item{&p, p, count * sizeof(T)};
        lay.array(p, count);
    }
    // arrays of `count` elements each, one behind the other
    template <typename... Ts>
    void brings(ScratchLayout& lay, uint64_t count, const Ts*&... ps) { (bring(lay, ps, count), ...); }

    int count() const { return used_; }
    void item(int i, void*& to, const void*& from, uint64_t& bytes) const {
        std::memcpy(&to, item_[i].var, sizeof(to));
        from = item_[i].from;
        bytes = item_[i].bytes;
    }

private:
    struct Item {
        const void* var;  // a const T*& of the caller's: the device copy once the block is placed
        const void* from;
        uint64_t bytes;
    };
    Item item_[ScratchLayout::MAX_ARRAYS];
    int used_ = 0;
};

}  // namespace hnswgpu
