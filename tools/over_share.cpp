// Share of overflowed keys and of set overflow-bitmap bits in a tokenizer's cuckoo merge
// table (DevTables::seg_over): the host build of tokenizer.cpp (build_cuckoo /
// build_cuckoo_mid / cuckoo_over) replayed on the accepted merges, in their insertion order.
// Input (stdin): lines "a b rank new_id" as tools/over_share.py writes them.
//   g++ -O2 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/over_share.cpp -o /tmp/over_share
#include <algorithm>
#include <cstdio>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../tokenizer-zig_amd/csrc/tables.hpp"

using Merges = std::unordered_map<uint64_t, std::pair<uint32_t, uint32_t>>;

static uint32_t pow2_bits(size_t n) {
    uint32_t bits = 4;
    while (((size_t)1 << bits) < n) ++bits;
    return bits;
}

template <class Slot, class Buckets>
static bool build(const Merges& merges, uint32_t bits, std::vector<uint2>& tab, Slot slot, Buckets buckets) {
    tab.assign((size_t)2 << bits, uint2{tkz::EMPTY32, tkz::EMPTY32});
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    for (auto& kv : merges) {
        uint2 cur = slot(kv);
        uint32_t b1, b2;
        buckets(cur, b1, b2);
        bool placed = false;
        for (uint32_t bk : {b1, b2})
            for (int s = 0; s < 2 && !placed; ++s)
                if (tab[2 * bk + s].x == tkz::EMPTY32) { tab[2 * bk + s] = cur; placed = true; }
        uint32_t bk = b1;
        for (int it = 0; it < 4096 && !placed; ++it) {
            rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
            std::swap(cur, tab[2 * bk + (rng & 1)]);
            uint32_t c1, c2;
            buckets(cur, c1, c2);
            bk = bk == c1 ? c2 : c1;
            for (int s = 0; s < 2 && !placed; ++s)
                if (tab[2 * bk + s].x == tkz::EMPTY32) { tab[2 * bk + s] = cur; placed = true; }
        }
        if (!placed) return false;
    }
    return true;
}

int main() {
    Merges merges;
    uint32_t a, b, rank, nid, max_id = 0;
    size_t accepted = 0;
    while (scanf("%u %u %u %u", &a, &b, &rank, &nid) == 4) {
        merges[((uint64_t)a << 32) | b] = {rank, nid};
        max_id = std::max({max_id, a, b, nid});
        ++accepted;
    }
    const bool compact = max_id < 0xFFFFu && accepted < 0xFFFFu;
    if (!compact && max_id >= (1u << 20) - 1) { printf("wide table: no cuckoo table\n"); return 0; }
    uint32_t bits = pow2_bits(merges.size() + 2);
    std::vector<uint2> tab;
    if (compact) {
        auto buckets = [&](const uint2& s, uint32_t& b1, uint32_t& b2) { tkz::merge_buckets_compact(s.x, bits, b1, b2); };
        auto slot = [](const Merges::value_type& kv) {
            return uint2{((uint32_t)(kv.first >> 32) << 16) | (uint32_t)kv.first, (kv.second.first << 16) | kv.second.second};
        };
        while (!build(merges, bits, tab, slot, buckets)) ++bits;
    } else {
        auto buckets = [&](const uint2& s, uint32_t& b1, uint32_t& b2) {
            tkz::merge_buckets_mid(s.x & 0xFFFFFu, (s.x >> 20) | ((s.y & 0xFFu) << 12), bits, b1, b2);
        };
        auto slot = [](const Merges::value_type& kv) {
            return tkz::mid_slot((uint32_t)(kv.first >> 32), (uint32_t)kv.first, kv.second.first);
        };
        while (!build(merges, bits, tab, slot, buckets)) ++bits;
    }
    std::vector<uint8_t> over((size_t)1 << bits, 0);
    size_t second = 0;
    for (size_t i = 0; i < tab.size(); ++i) {
        if (tab[i].x == tkz::EMPTY32) continue;
        uint32_t b1, b2;
        if (compact) tkz::merge_buckets_compact(tab[i].x, bits, b1, b2);
        else tkz::merge_buckets_mid(tab[i].x & 0xFFFFFu, (tab[i].x >> 20) | ((tab[i].y & 0xFFu) << 12), bits, b1, b2);
        if (i / 2 != b1) { over[b1] = 1; ++second; }
    }
    size_t set = 0, keyed = 0;  // keyed: keys whose first bucket's bit is set (their probes load two buckets)
    for (auto v : over) set += v;
    for (size_t i = 0; i < tab.size(); ++i) {
        if (tab[i].x == tkz::EMPTY32) continue;
        uint32_t b1, b2;
        if (compact) tkz::merge_buckets_compact(tab[i].x, bits, b1, b2);
        else tkz::merge_buckets_mid(tab[i].x & 0xFFFFFu, (tab[i].x >> 20) | ((tab[i].y & 0xFFu) << 12), bits, b1, b2);
        keyed += over[b1];
    }
    printf("%s table: %zu keys, 2^%u buckets (bitmap %zu B); %zu keys (%.1f %%) in their second bucket; "
           "%zu bits set (%.1f %%); %.1f %% of the keys probe two buckets\n",
           compact ? "compact" : "mid", merges.size(), bits, ((size_t)1 << bits) / 8, second,
           100.0 * second / merges.size(), set, 100.0 * set / ((size_t)1 << bits), 100.0 * keyed / merges.size());
    return 0;
}
