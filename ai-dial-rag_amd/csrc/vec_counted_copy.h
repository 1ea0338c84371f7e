// The last step of the vector searches' host forms that calls nothing of HIP: a [b, k] result array goes
// from the staging buffer to the caller's, the listed entries of each query only.  The kernels write the first count[q]
// entries of a row and nothing after them, so what lies past the count in the staging buffer is what an earlier call
// left there.  vec_index.hip includes it; any C++ compiler builds it alone (tests/counted_copy_check.cpp does).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace mir {

// Copies the first clamp(count[q], 0, k) elements of each of the b rows of k elements of `elem` bytes from `src` (b k
// elements, contiguous) to the same places of `dst`; every other byte of `dst` stays as it was.  A null `dst` is
// skipped.  When every count is k or more - the usual call - it is ONE memcpy of the whole array.
inline void counted_copy(void *dst, const void *src, const int32_t *count, int64_t b, int64_t k, size_t elem) {
    if (!dst || b <= 0 || k <= 0) return;
    int64_t full = 0;
    while (full < b && count[full] >= k) ++full;
    char *to = static_cast<char *>(dst);
    const char *from = static_cast<const char *>(src);
    const size_t row = (size_t)k * elem;
    if (full) std::memcpy(to, from, (size_t)full * row);  // the leading full rows (all of them, as a rule) in one piece
    for (int64_t q = full; q < b; ++q) {
        const int64_t n = count[q] < 0 ? 0 : count[q] < k ? count[q] : k;
        if (n) std::memcpy(to + (size_t)q * row, from + (size_t)q * row, (size_t)n * elem);
    }
}

}  // namespace mir
