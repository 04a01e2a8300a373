// lime_extents.h -- the free list of a reserved arena (lime_alloc.cpp: BlockCache, lime_reserve): first fit over offset-sorted extents, sizes in
// whole granules, a returned piece merged with its neighbours.  Pure bookkeeping without HIP: tests/test_extents_cpu.py builds it with g++ alone.
#pragma once
#include <stddef.h>
#include <vector>

namespace lime_host __attribute__((visibility("hidden"))) {
struct Extents {
    struct Ext { size_t off, bytes; };
    static constexpr size_t NONE = (size_t)-1;
    size_t gran;
    std::vector<Ext> free_;                                 // offset-sorted, non-overlapping, no two adjacent
    Extents(size_t bytes, size_t granule) : gran(granule), free_{Ext{0, bytes}} {}
    // `bytes` rounded up to the granule from the lowest extent that holds them: the piece's offset (NONE: nothing fits), *got = its size
    size_t take(size_t bytes, size_t *got)
    {
        const size_t want = (bytes + gran - 1) / gran * gran;
        for (size_t i = 0; i < free_.size(); ++i)
            if (free_[i].bytes >= want) {
                const size_t off = free_[i].off;
                if (free_[i].bytes == want) free_.erase(free_.begin() + (long)i);
                else { free_[i].off += want; free_[i].bytes -= want; }
                *got = want;
                return off;
            }
        return NONE;
    }
    // a piece take() handed out (its offset and the size take reported) is free again
    void give(size_t off, size_t bytes)
    {
        size_t i = 0;
        while (i < free_.size() && free_[i].off < off) ++i;
        free_.insert(free_.begin() + (long)i, Ext{off, bytes});
        if (i + 1 < free_.size() && free_[i].off + free_[i].bytes == free_[i + 1].off) { free_[i].bytes += free_[i + 1].bytes; free_.erase(free_.begin() + (long)i + 1); }
        if (i > 0 && free_[i - 1].off + free_[i - 1].bytes == free_[i].off) { free_[i - 1].bytes += free_[i].bytes; free_.erase(free_.begin() + (long)i); }
    }
};
}
