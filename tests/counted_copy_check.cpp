// Stand-alone check of csrc/vec_counted_copy.h (no HIP, no GPU): the copy that brings a [b, k] result array of a vector
// search's host form to the caller.  tests/test_counted_copy.py builds it with the host compiler and the address and
// undefined-behaviour sanitizers, and runs it.  Source and destination are exact heap allocations, so a read or a write
// past either is the sanitizer's finding as well as the guards'.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vec_counted_copy.h"

static int failures = 0;
static long copies = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);       \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

static const size_t kGuard = 64;
static unsigned char src_byte(size_t i) { return (unsigned char)(0x80 | (i * 7 + 3) % 0x7f); }  // high bit set
static unsigned char dst_byte(size_t i) { return (unsigned char)((i * 5 + 1) % 0x7f); }         // high bit clear
static const unsigned char kGuardByte = 0x7f;                                                   // neither pattern has it

static int64_t clamp(int64_t c, int64_t k) { return c < 0 ? 0 : c < k ? c : k; }

// one copy with the given counts: exactly the first clamp(count[q], 0, k) elements of each row become the source's
static void check_one(int64_t b, int64_t k, size_t elem, const std::vector<int32_t> &count) {
    const size_t bytes = (size_t)b * (size_t)k * elem;
    std::vector<unsigned char> src(bytes), dst(kGuard + bytes + kGuard);
    for (size_t i = 0; i < bytes; ++i) src[i] = src_byte(i);
    for (size_t i = 0; i < kGuard; ++i) dst[i] = dst[kGuard + bytes + i] = kGuardByte;
    for (size_t i = 0; i < bytes; ++i) dst[kGuard + i] = dst_byte(i);
    const std::vector<unsigned char> src_before = src;
    const std::vector<int32_t> count_before = count;
    mir::counted_copy(dst.data() + kGuard, src.data(), count.data(), b, k, elem);
    ++copies;
    bool guards = true, listed = true, rest = true;
    for (size_t i = 0; i < kGuard; ++i) guards = guards && dst[i] == kGuardByte && dst[kGuard + bytes + i] == kGuardByte;
    for (int64_t q = 0; q < b; ++q) {
        const size_t row = (size_t)q * (size_t)k * elem, cut = (size_t)clamp(count[(size_t)q], k) * elem;
        for (size_t i = 0; i < (size_t)k * elem; ++i) {
            const unsigned char got = dst[kGuard + row + i];
            if (i < cut) listed = listed && got == src_byte(row + i);
            else rest = rest && got == dst_byte(row + i);
        }
    }
    CHECK(guards);
    CHECK(listed);
    CHECK(rest);
    CHECK(src == src_before);
    CHECK(count == count_before);
    // a null destination is skipped (an array the caller did not ask for); the sanitizer would see a write through it
    mir::counted_copy(nullptr, src.data(), count.data(), b, k, elem);
    CHECK(src == src_before);
}

int main() {
    const int64_t bs[] = {0, 1, 3, 257}, ks[] = {1, 5, 70};
    const size_t elems[] = {4, 8};
    uint64_t state = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {  // xorshift64: the same draws on every run
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        return state;
    };
    for (int64_t b : bs)
        for (int64_t k : ks)
            for (size_t elem : elems) {
                const int32_t values[] = {-7, INT32_MIN, 0, 1, (int32_t)k - 1, (int32_t)k, (int32_t)k + 1, INT32_MAX};
                const size_t nv = sizeof(values) / sizeof(values[0]);
                for (int32_t v : values) check_one(b, k, elem, std::vector<int32_t>((size_t)b, v));  // every row the same count
                for (int round = 0; round < 8; ++round) {  // mixed: drawn per row
                    std::vector<int32_t> count((size_t)b);
                    for (auto &c : count) c = values[next() % nv];
                    check_one(b, k, elem, count);
                }
                // full rows first and a short one last, and the reverse: where the one-memcpy prefix ends
                if (b > 1) {
                    std::vector<int32_t> count((size_t)b, (int32_t)k);
                    count[(size_t)b - 1] = (int32_t)k - 1;
                    check_one(b, k, elem, count);
                    count.assign((size_t)b, (int32_t)k);
                    count[0] = 0;
                    check_one(b, k, elem, count);
                }
            }
    // b or k that is not positive: nothing is touched, whatever the pointers are
    int32_t one = 1;
    unsigned char cell[8] = {1, 2, 3, 4, 5, 6, 7, 8}, same[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    mir::counted_copy(cell, cell, &one, -1, 5, 8);
    mir::counted_copy(cell, cell, &one, 1, 0, 8);
    CHECK(std::memcmp(cell, same, 8) == 0);
    if (failures) {
        std::printf("counted_copy: %d failures\n", failures);
        return 1;
    }
    std::printf("counted_copy: ok, %ld copies checked\n", copies);
    return 0;
}
