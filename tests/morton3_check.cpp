// morton3_check.cpp -- a stand-alone program (tests/test_terrain_edits_cpu.py builds it with g++ under AddressSanitizer + UBSan
// and runs it): csrc/morton3.hpp's spread3 / compact3, the host instances of what the edit kernels run, against a loop that
// moves one bit at a time.  All 2^21 inputs of spread3; compact3(spread3(x) << s) for s = 0, 1, 2; compact3 of words whose other
// two lanes (and bit 63) hold junk.  The suite's trees give a brick coordinate 3 bits; the << 32 and << 16 stages first move a
// set bit at 11 and 6 bits.
#include <stdint.h>
#include <stdio.h>

#include "morton3.hpp"

static uint64_t spread_by_bits(uint64_t x) {
    uint64_t out = 0;
    for (int k = 0; k < 21; ++k) out |= ((x >> k) & 1ULL) << (3 * k);
    return out;
}

static uint32_t compact_by_bits(uint64_t x) {
    uint32_t out = 0;
    for (int k = 0; k < 21; ++k) out |= (uint32_t)((x >> (3 * k)) & 1ULL) << k;
    return out;
}

int main() {
    long long spreads = 0, round_trips = 0, junk_words = 0, above_20_bits = 0;
    uint64_t rnd = 0x9e3779b97f4a7c15ULL;
    for (uint64_t x = 0; x < (1ULL << 21); ++x) {
        const uint64_t s = vrc::spread3(x), want = spread_by_bits(x);
        if (s != want) {
            printf("spread3(%#llx) = %#llx, by bits %#llx\n", (unsigned long long)x, (unsigned long long)s, (unsigned long long)want);
            return 1;
        }
        ++spreads;
        // bits above the 21 are dropped, not smeared into the lanes
        if (vrc::spread3(x | (x << 21) | (1ULL << 63)) != want) {
            printf("spread3 of %#llx with bits above 20: wrong\n", (unsigned long long)x);
            return 1;
        }
        ++above_20_bits;
        for (int shift = 0; shift < 3; ++shift) {
            // a coordinate in lane `shift` comes back from there, and lane 0 does not see it
            if (vrc::compact3((s << shift) >> shift) != (uint32_t)x || vrc::compact3(s << shift) != (shift == 0 ? (uint32_t)x : 0u)) {
                printf("round trip of %#llx in lane %d: wrong\n", (unsigned long long)x, shift);
                return 2;
            }
            // the key as the kernels read it back: compact3(key >> shift) with the other two coordinates in their lanes
            rnd = rnd * 6364136223846793005ULL + 1442695040888963407ULL;
            const uint64_t a = (rnd >> 11) & 0x1fffff, b = (rnd >> 40) & 0x1fffff;
            const uint64_t lanes[3] = {shift == 0 ? x : a, shift == 1 ? x : (shift == 0 ? a : b), shift == 2 ? x : b};
            const uint64_t key = spread_by_bits(lanes[0]) | spread_by_bits(lanes[1]) << 1 | spread_by_bits(lanes[2]) << 2;
            if ((vrc::spread3(lanes[0]) | vrc::spread3(lanes[1]) << 1 | vrc::spread3(lanes[2]) << 2) != key) {
                printf("the key of (%#llx, %#llx, %#llx): wrong\n", (unsigned long long)lanes[0], (unsigned long long)lanes[1], (unsigned long long)lanes[2]);
                return 3;
            }
            for (int lane = 0; lane < 3; ++lane) {
                const uint32_t got = vrc::compact3(key >> lane);
                if (got != (uint32_t)lanes[lane] || got != compact_by_bits(key >> lane)) {
                    printf("compact3(%#llx >> %d) = %#x, want %#llx\n", (unsigned long long)key, lane, got, (unsigned long long)lanes[lane]);
                    return 3;
                }
                ++junk_words;
            }
            // ... and with bit 63 set, which no lane owns
            if (vrc::compact3(key | (1ULL << 63)) != (uint32_t)lanes[0]) {
                printf("compact3 of %#llx with bit 63 set: wrong\n", (unsigned long long)key);
                return 4;
            }
            ++round_trips;
        }
    }
    printf("morton3 ok: spreads %lld, round trips %lld, junk words %lld, above 20 bits %lld\n", spreads, round_trips, junk_words, above_20_bits);
    return 0;
}
