// extents_check.cpp -- stand-alone check of lime_amd/csrc/lime_extents.h (the free list of a reserved arena), built and run by
// tests/test_extents_cpu.py with g++ and -fsanitize=address,undefined.  No HIP.  Exit code 0 and "ok" on stdout: every check held.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "lime_extents.h"

using lime_host::Extents;

static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++g_bad; } } while (0)

static const size_t G = (size_t)2 << 20;                    // the arenas' granule

static bool is_list(const Extents &e, std::initializer_list<Extents::Ext> want)
{
    if (e.free_.size() != want.size()) return false;
    size_t i = 0;
    for (const Extents::Ext &w : want) { if (e.free_[i].off != w.off || e.free_[i].bytes != w.bytes) return false; ++i; }
    return true;
}

// sorted by offset, no overlap, no two adjacent (adjacent ones would have been merged), nothing empty, nothing past the end
static bool well_formed(const Extents &e, size_t total)
{
    for (size_t i = 0; i < e.free_.size(); ++i) {
        if (!e.free_[i].bytes || e.free_[i].off % G || e.free_[i].bytes % G || e.free_[i].off + e.free_[i].bytes > total) return false;
        if (i && e.free_[i - 1].off + e.free_[i - 1].bytes >= e.free_[i].off) return false;
    }
    return true;
}

static void fixed_cases()
{
    size_t got = 0;
    {   // sizes round up to the granule; first fit takes the lowest offset that fits; an exact fit removes the extent
        Extents e(16 * G, G);
        CHECK(e.take(1, &got) == 0 && got == G);
        CHECK(e.take(G + 1, &got) == G && got == 2 * G);
        CHECK(e.take(3 * G, &got) == 3 * G && got == 3 * G);
        CHECK(e.take(2 * G, &got) == 6 * G && got == 2 * G);
        CHECK(is_list(e, {{8 * G, 8 * G}}));
        e.give(G, 2 * G);                                    // a hole of 2 below a hole of ... below the tail
        e.give(6 * G, 2 * G);                                // merges with its right neighbour (the tail)
        CHECK(is_list(e, {{G, 2 * G}, {6 * G, 10 * G}}));
        CHECK(e.take(3 * G, &got) == 6 * G && got == 3 * G); // the hole of 2 at the lower offset does not fit: the next one
        CHECK(e.take(2 * G - 5, &got) == G && got == 2 * G); // exact (after rounding): the extent is gone
        CHECK(is_list(e, {{9 * G, 7 * G}}));
        CHECK(e.take(8 * G, &got) == Extents::NONE);         // nothing fits: the list is untouched
        CHECK(is_list(e, {{9 * G, 7 * G}}));
        CHECK(e.take(7 * G, &got) == 9 * G && e.free_.empty());
        CHECK(e.take(1, &got) == Extents::NONE);
    }
    {   // a returned piece merges with its left neighbour, with its right neighbour, with both
        Extents e(8 * G, G);
        size_t off[8];
        for (int k = 0; k < 8; ++k) { off[k] = e.take(G, &got); CHECK(off[k] == (size_t)k * G && got == G); }
        CHECK(e.free_.empty());
        e.give(off[1], G);
        e.give(off[5], G);
        CHECK(is_list(e, {{G, G}, {5 * G, G}}));
        e.give(off[2], G);                                   // left neighbour
        CHECK(is_list(e, {{G, 2 * G}, {5 * G, G}}));
        e.give(off[4], G);                                   // right neighbour
        CHECK(is_list(e, {{G, 2 * G}, {4 * G, 2 * G}}));
        e.give(off[3], G);                                   // both
        CHECK(is_list(e, {{G, 5 * G}}));
        e.give(off[7], G);                                   // neither
        CHECK(is_list(e, {{G, 5 * G}, {7 * G, G}}));
        e.give(off[0], G); e.give(off[6], G);
        CHECK(is_list(e, {{0, 8 * G}}));
    }
}

// a few thousand random takes and gives against a bitmap of granules (first fit by brute force)
static void random_walk(uint64_t seed, size_t n_gran, int steps)
{
    uint64_t s = seed;
    auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
    const size_t total = n_gran * G;
    Extents e(total, G);
    std::vector<uint8_t> used(n_gran, 0);
    struct Piece { size_t off, bytes; };
    std::vector<Piece> live;
    for (int step = 0; step < steps; ++step) {
        if (live.empty() || rnd() % 100 < 55) {
            const size_t bytes = (size_t)(rnd() % 12 + 1) * G - rnd() % G;     // 1 .. 12 granules after rounding
            const size_t g = (bytes + G - 1) / G;
            size_t model = Extents::NONE;
            for (size_t lo = 0, run = 0, i = 0; i < n_gran; ++i) {
                if (used[i]) { run = 0; lo = i + 1; continue; }
                if (++run == g) { model = lo * G; break; }
            }
            size_t got = 0;
            const size_t off = e.take(bytes, &got);
            CHECK(off == model);
            if (off != Extents::NONE) {
                CHECK(got == g * G);
                for (size_t i = 0; i < g; ++i) { CHECK(!used[off / G + i]); used[off / G + i] = 1; }
                live.push_back(Piece{off, got});
            }
        } else {
            const size_t k = rnd() % live.size();
            const Piece p = live[k];
            live[k] = live.back(); live.pop_back();
            for (size_t i = 0; i < p.bytes / G; ++i) used[p.off / G + i] = 0;
            e.give(p.off, p.bytes);
        }
        CHECK(well_formed(e, total));
        size_t free_model = 0, free_list = 0;
        for (uint8_t u : used) free_model += u ? 0 : G;
        for (const Extents::Ext &x : e.free_) { free_list += x.bytes; for (size_t i = 0; i < x.bytes / G; ++i) CHECK(!used[x.off / G + i]); }
        CHECK(free_model == free_list);
        if (g_bad) return;
    }
    while (!live.empty()) { e.give(live.back().off, live.back().bytes); live.pop_back(); CHECK(well_formed(e, total)); }
    CHECK(e.free_.size() == 1 && e.free_[0].off == 0 && e.free_[0].bytes == total);     // the single extent it started as
}

int main()
{
    fixed_cases();
    random_walk(1, 64, 4000);
    random_walk(2, 257, 4000);
    random_walk(3, 13, 2000);                                // mostly full: takes that find nothing
    if (g_bad) { printf("%d check(s) failed\n", g_bad); return 1; }
    printf("ok\n");
    return 0;
}
