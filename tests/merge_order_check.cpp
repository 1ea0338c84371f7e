// csrc/merge_order.h on the host alone (tests/test_oracle_merge.py builds this with the address and undefined-behaviour
// sanitizers and runs it): the order that both merge kernels and mir_topk_merge_host share is a strict weak order - what
// std::sort demands and the comparator it replaces was not once a score is NaN - it is total over distinct rows, and it
// places NaN, the zeros and the infinities where np.argsort(kind="stable") (reversed for descending) places them.
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "merge_order.h"

struct Item {
    double d;
    int64_t r;
};

static double from_bits(uint64_t u) {
    double d;
    std::memcpy(&d, &u, 8);
    return d;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity();
    const double values[] = {0.0, -0.0, 1.0, -1.0, inf, -inf, 5e-324, -5e-324, 0.5, 1e308,
                             from_bits(0x7FF8000000000000ull), from_bits(0xFFF8000000000001ull), from_bits(~0ull)};
    const int64_t rows[] = {0, 1, 0x7FFFFFFF, 0x80000000ll, 1ll << 32, (1ll << 32) + 1, (5ll << 32) + 1, 1ll << 40};
    std::vector<Item> items;
    int nv = 0;  // every item its own row, as in one query of a merge: -0 and +0, or two NaNs, never share one
    for (double d : values) {
        for (int64_t r : rows) items.push_back({d, r + 16 * nv});
        ++nv;
    }
    const size_t n = items.size();
    for (int desc = 0; desc < 2; ++desc) {
        auto before = [desc](const Item &a, const Item &c) {
            return mir::merge_before(mir::merge_order_key(a.d, desc), a.r, mir::merge_order_key(c.d, desc), c.r, desc);
        };
        for (size_t i = 0; i < n; ++i) {
            assert(!before(items[i], items[i]));
            for (size_t j = 0; j < n; ++j) {
                const bool ij = before(items[i], items[j]), ji = before(items[j], items[i]);
                assert(!(ij && ji));
                assert(i == j || ij || ji);  // distinct rows are never equivalent: the merge is deterministic
                for (size_t l = 0; l < n; ++l)
                    if (ij && before(items[j], items[l])) assert(before(items[i], items[l]));
            }
        }
        // the named places: NaN after every number ascending and before every number descending, whatever its sign or
        // payload; -0 = +0 and NaN = NaN fall to the row, the lower one ascending, the higher one descending
        const Item nan_lo{from_bits(~0ull), 3}, nan_hi{from_bits(0x7FF8000000000000ull), 4};
        const Item pinf{inf, 9}, ninf{-inf, 9}, mzero{-0.0, 7}, pzero{0.0, 8}, tiny{5e-324, 1};
        assert(before(pinf, nan_lo) == !desc && before(nan_lo, ninf) == !!desc);
        assert(before(nan_lo, nan_hi) == !desc && before(nan_hi, nan_lo) == !!desc);
        assert(before(mzero, pzero) == !desc && before(pzero, mzero) == !!desc);
        assert(before(pzero, tiny) == !desc && before(ninf, mzero) == !desc);
        // std::sort on it, from several starting orders, gives one result
        std::vector<Item> a = items, c = items;
        std::reverse(c.begin(), c.end());
        std::rotate(c.begin(), c.begin() + 17, c.end());
        std::sort(a.begin(), a.end(), before);
        std::sort(c.begin(), c.end(), before);
        for (size_t i = 0; i < n; ++i) {
            assert(a[i].r == c[i].r && std::memcmp(&a[i].d, &c[i].d, 8) == 0);
            if (i) assert(before(a[i - 1], a[i]));
        }
        assert((a[0].d != a[0].d) == !!desc && (a[n - 1].d != a[n - 1].d) == !desc);
    }
    std::printf("merge_order: ok (%zu items)\n", n);
    return 0;
}
