// Stand-alone check of csrc/vec_scoped_layout.h (no HIP, no GPU): what the scoped vector searches' host forms refuse, how
// scopes are cut, the shared search's plan and slab counts, and the workspace layout.  tests/test_vec_scoped_layout.py
// builds it with the host compiler and the address and undefined-behaviour sanitizers, and runs it.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "vec_scoped_layout.h"

using namespace mir;

// the library's set_error lives in vec_index.hip; this program keeps the text where the checks can read it
static char g_err[512] = "";
void mir::set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static int failures = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);       \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

static bool said(const char *part) { return std::strstr(g_err, part) != nullptr; }

// the kernels' limits, restated (vec_kernels.h, vec_kernels_scoped.h, vec_kernels_shared.h)
constexpr int kRound = 64, kWaves = 4, kScopedMaxP = 64, kSharedMaxP = 256;

static void check_ptr_arrays() {
    const std::vector<std::vector<int32_t>> good = {{0}, {0, 0, 3}, {0, 2, 3}};
    for (const auto &p : good) CHECK(check_ptr_array(p.data(), (int)p.size() - 1, "scope_ptr", "query") == MIR_OK);
    const int32_t from_one[] = {1, 1, 2}, down[] = {0, 2, 1};
    CHECK(check_ptr_array(from_one, 2, "scope_ptr", "query") == MIR_ERR_INVALID);
    CHECK(std::string(g_err) == "scope_ptr[0]=1 must be 0");
    CHECK(check_ptr_array(from_one, 2, "group_ptr", "group") == MIR_ERR_INVALID);
    CHECK(std::string(g_err) == "group_ptr[0]=1 must be 0");
    CHECK(check_ptr_array(down, 2, "scope_ptr", "query") == MIR_ERR_INVALID);
    CHECK(std::string(g_err) == "scope_ptr decreases at query 1");
    CHECK(check_ptr_array(down, 2, "scope_ptr", "group") == MIR_ERR_INVALID);
    CHECK(std::string(g_err) == "scope_ptr decreases at group 1");
    CHECK(check_ptr_array(down, 2, "group_ptr", "group") == MIR_ERR_INVALID);
    CHECK(std::string(g_err) == "group_ptr decreases at group 1");
}

static int32_t walk_ranges(const std::vector<int32_t> &sp, const std::vector<int64_t> &b, const std::vector<int64_t> &e, int64_t n,
                           ScopeRows *out) {
    return walk_scopes(sp.data(), (int)sp.size() - 1, "query", nullptr, range_rows(b.data(), e.data(), n), out);
}

static void check_walk_ranges() {
    ScopeRows r{};
    CHECK(walk_ranges({0, 1, 2}, {0, 50}, {50, 100}, 100, &r) == MIR_OK && r.nseg == 2 && r.max_rows == 50);
    // an empty scope, an empty segment; a scope of two segments is their sum
    CHECK(walk_ranges({0, 0, 1}, {50}, {50}, 100, &r) == MIR_OK && r.nseg == 1 && r.max_rows == 1);
    CHECK(walk_ranges({0, 0, 0}, {}, {}, 100, &r) == MIR_OK && r.nseg == 0 && r.max_rows == 1);
    CHECK(walk_ranges({0, 2, 3}, {0, 90, 5}, {30, 100, 25}, 100, &r) == MIR_OK && r.nseg == 3 && r.max_rows == 40);
    // the three ways out of the index, each the second segment of query 1
    CHECK(walk_ranges({0, 1, 3}, {0, 0, -1}, {5, 5, 5}, 100, &r) == MIR_ERR_INVALID);
    CHECK(std::string(g_err) == "segment 1 of query 1 is [-1, 5): not inside 0 <= begin <= end <= n=100");
    CHECK(walk_ranges({0, 1, 3}, {0, 0, 60}, {5, 5, 50}, 100, &r) == MIR_ERR_INVALID);
    CHECK(std::string(g_err) == "segment 1 of query 1 is [60, 50): not inside 0 <= begin <= end <= n=100");
    CHECK(walk_ranges({0, 1, 3}, {0, 0, 0}, {5, 5, 101}, 100, &r) == MIR_ERR_INVALID);
    CHECK(std::string(g_err) == "segment 1 of query 1 is [0, 101): not inside 0 <= begin <= end <= n=100");
    // 2^32 rows or more: [0, 70 000) listed 61 357 times is refused, 61 356 times (4 294 920 000 rows) is not
    const int many = 61357;
    const std::vector<int64_t> b0((size_t)many + 1, 0), e0((size_t)many + 1, 70000);
    CHECK(walk_ranges({0, 1, 1 + many}, b0, e0, 70000, &r) == MIR_ERR_INVALID);
    CHECK(std::string(g_err) == "the scope of query 1 holds 2^32 rows or more" && said("2^32"));
    CHECK(walk_ranges({0, many - 1}, b0, e0, 70000, &r) == MIR_OK && r.nseg == (size_t)many - 1 && r.max_rows == 4294920000ull);
}

static void check_walk_blocks() {
    // lengths from an array; a negative one is a block the route refuses.  `table` stands for the descriptor table.
    std::vector<int64_t> len = {10, 20, -1, 30}, table(len.size(), -7);
    auto rows_of = [&](int t, int ordinal, int i, uint64_t *rows) -> int32_t {
        if (len[(size_t)t] < 0) {
            set_error("block %d of group %d is marked", ordinal, i);
            return MIR_ERR_UNSUPPORTED;
        }
        table[(size_t)t] = len[(size_t)t];
        *rows = (uint64_t)len[(size_t)t];
        return MIR_OK;
    };
    ScopeRows r{};
    const int32_t sp[] = {0, 1, 4};
    CHECK(walk_scopes(sp, 2, "group", nullptr, rows_of, &r) == MIR_ERR_UNSUPPORTED);  // the callable's own code, and its text
    CHECK(std::string(g_err) == "block 1 of group 1 is marked");
    CHECK((table == std::vector<int64_t>{10, 20, -7, -7}));
    len[2] = 5;
    CHECK(walk_scopes(sp, 2, "group", nullptr, rows_of, &r) == MIR_OK && r.nseg == 4 && r.max_rows == 55);
    CHECK((table == std::vector<int64_t>{10, 20, 5, 30}));
    // the refusal names the unit it was given
    len = {0, 0x7fffffff, 0x7fffffff, 2};  // group 1: 2^32 rows exactly
    CHECK(walk_scopes(sp, 2, "group", nullptr, rows_of, &r) == MIR_ERR_INVALID);
    CHECK(std::string(g_err) == "the scope of group 1 holds 2^32 rows or more");
    // the shared search: groups of 2, 0 and 1 queries over scopes of 10, 1000 and 7 rows - nobody searches the 1000
    len = {10, 1000, 7};
    table.assign(3, 0);
    const int32_t one_each[] = {0, 1, 2, 3}, group_ptr[] = {0, 2, 2, 3};
    CHECK(walk_scopes(one_each, 3, "group", group_ptr, rows_of, &r) == MIR_OK && r.nseg == 3 && r.max_rows == 10);
    CHECK(walk_scopes(one_each, 3, "query", nullptr, rows_of, &r) == MIR_OK && r.max_rows == 1000);
}

static void check_slabs() {
    const int32_t group_ptr[] = {0, 33, 50, 50, 66, 81};  // groups of 33, 17, 0, 16, 15 queries
    CHECK(shared_slab_count(group_ptr, 5, 16) == 3 + 2 + 0 + 1 + 1);
    CHECK(shared_max_slabs(81, 5, 16) == 6 + 5);
    CHECK(shared_max_slabs(81, 5, 16) >= shared_slab_count(group_ptr, 5, 16));
    CHECK(shared_slab_count(group_ptr, 0, 16) == 0);
    CHECK(shared_max_slabs(0x7fffffff, 0x7fffffff, 16) == 0x7fffffff);
}

static void check_plan() {
    // bytes = qs (8 dpad [fragments in LDS] + 48 min(k, 64)), dpad = d rounded up to 16; the widest qs of 64, 32 whose bytes
    // stay within 64 KiB, else 16 with the fragments in LDS up to 144 KiB, else 16 without
    struct { int d, k, qs; bool qlds; size_t lds; } want[] = {
        {64, 7, 64, true, 54272},   {128, 7, 32, true, 43520},    {384, 7, 16, true, 54528},  {1024, 7, 16, true, 136448},
        {1024, 64, 16, false, 49152}, {1024, 200, 16, false, 49152}, {383, 7, 16, true, 54528},
    };
    for (const auto &w : want) {
        const SharedPlan p = shared_plan(w.d, w.k, kRound, kWaves);
        CHECK(p.qs == w.qs && p.qlds == w.qlds && p.lds == w.lds);
        const size_t dpad = ((size_t)w.d + 15) / 16 * 16, kk = (size_t)(w.k < 64 ? w.k : 64);
        CHECK(p.lds == (size_t)p.qs * ((p.qlds ? 8 * dpad : 0) + 48 * kk));
    }
}

static void check_splits() {
    CHECK(scoped_split(256, 1, 1000000, kScopedMaxP) == 64);
    CHECK(scoped_split(256, 256, 1000, kScopedMaxP) == 4);
    CHECK(scoped_split(256, 1, 100, kScopedMaxP) == 2);
    CHECK(scoped_split(256, 5000, 1000000, kScopedMaxP) == 1);
    CHECK(scoped_split(256, 5000, 0, kScopedMaxP) == 1);
    CHECK(scoped_split(256, 1, 0, kScopedMaxP) == 64);  // the device form: the scopes are not seen
    CHECK(scoped_split(0, 1, 0, kScopedMaxP) == 4);     // (a CU count of 0 is taken as 1)
    CHECK(shared_split(256, 1, 0, kSharedMaxP) == 256);
    CHECK(shared_split(256, 1, 10000, kSharedMaxP) == 20);
    CHECK(shared_split(256, 2000, 0, kSharedMaxP) == 1);
    CHECK(shared_split(256, 2000, 10000, kSharedMaxP) == 1);
    CHECK(shared_split(256, 0, 0, kSharedMaxP) == 256);  // no slab: no division by zero
}

static size_t up(size_t x) { return (x + 255) & ~(size_t)255; }

template <typename T>
static size_t at(const T *p, const char *base) { return (size_t)(reinterpret_cast<const char *>(p) - base); }

// route 0: row ranges, 1: blocks, 2: the shared search over (n_groups, slabs) = (2, 3)
static void check_carve(int b, int k, int d, int P, size_t nseg, bool host, int route, size_t parent_bytes) {
    ScopedShape s{b, k, d, P, nseg, host, route > 0};
    if (route == 2) {
        s.n_groups = 2;
        s.max_slabs = 3;
    }
    const bool shared = route == 2;
    ScopedBuffers sb;
    const size_t bytes = carve_scoped(sb, nullptr, s, kRound);
    CHECK(bytes == parent_bytes);  // what this layout took before it moved here
    CHECK(sb.q == nullptr && sb.q_sq == nullptr && sb.part == nullptr && sb.out.flags == nullptr);
    std::vector<char> slab(bytes);
    const char *base = slab.data();
    CHECK(carve_scoped(sb, slab.data(), s, kRound) == bytes);
    const size_t B = (size_t)b, scopes = shared ? 2 : B;
    size_t o = 0;  // every piece starts at the next multiple of 256 after the one before it, in the documented order
    auto next = [&](size_t bytes_of_piece) {
        const size_t here = up(o);
        o = here + bytes_of_piece;
        return here;
    };
    if (host) {
        CHECK(at(sb.q, base) == next(B * d * 8) && at(sb.q, base) == 0);
        if (shared) CHECK(at(sb.group_ptr, base) == next((scopes + 1) * 4));
        else CHECK(sb.group_ptr == nullptr);
        CHECK(at(sb.scope_ptr, base) == next((scopes + 1) * 4));
        if (route == 0) {
            CHECK(at(sb.seg_begin, base) == next(nseg * 8));
            CHECK(at(sb.seg_end, base) == next(nseg * 8));
            CHECK(sb.table == nullptr);
        } else {
            CHECK(at(sb.table, base) == next(nseg * sizeof(mir_block_desc)));
            CHECK(sb.seg_begin == nullptr && sb.seg_end == nullptr);
        }
    } else {
        CHECK(!sb.q && !sb.group_ptr && !sb.scope_ptr && !sb.seg_begin && !sb.seg_end && !sb.table);
    }
    CHECK(sb.in_span == o);  // the host forms' one copy in: [q .. end of seg_end / table)
    CHECK(at(sb.q_sq, base) == next(B * 8));
    CHECK(at(sb.q_norm, base) == next(B * 8));
    CHECK(at(sb.arrive, base) == next(((shared ? 3 : B) + 1) / 2 * 8));  // one 32-bit counter per query, or per slab
    CHECK(at(sb.bound_dist, base) == next(B * 8));
    CHECK(at(sb.bound_pos, base) == next(B * 4));
    CHECK(at(sb.part, base) == next(P > 1 ? B * P * (size_t)(k < 64 ? k : 64) * 16 : 0));
    if (shared) {
        CHECK(at(sb.slabs, base) == next(3 * sizeof(SharedSlab)) && sizeof(SharedSlab) == 8);
        CHECK(at(sb.n_slabs, base) == next(4));
    } else {
        CHECK(sb.slabs == nullptr && sb.n_slabs == nullptr);
    }
    if (host) {  // the one copy out: [doc .. end of flags)
        CHECK(at(sb.out.doc, base) == next(B * k * 4));
        CHECK(at(sb.out.chunk, base) == next(B * k * 8));
        CHECK(at(sb.out.row, base) == next(B * k * 8));
        CHECK(at(sb.out.dist, base) == next(B * k * 8));
        CHECK(at(sb.out.count, base) == next(B * 4));
        CHECK(at(sb.out.flags, base) == next(B * 4));
    } else {
        CHECK(!sb.out.doc && !sb.out.chunk && !sb.out.row && !sb.out.dist && !sb.out.count && !sb.out.flags);
    }
    CHECK(bytes == o + 256);
}

int main() {
    check_ptr_arrays();
    check_walk_ranges();
    check_walk_blocks();
    check_slabs();
    check_plan();
    check_splits();
    // {b, k, d, P, nseg, host form, route, bytes}: the bytes are those of carve_scoped as it stood in vec_index.hip
    const size_t parent[][8] = {
        {1, 1, 8, 1, 0, 0, 0, 1536},        {1, 1, 8, 1, 0, 0, 1, 1536},        {1, 1, 8, 1, 0, 0, 2, 1796},
        {1, 1, 8, 1, 0, 1, 0, 3332},        {1, 1, 8, 1, 0, 1, 1, 3332},        {1, 1, 8, 1, 0, 1, 2, 4100},
        {3, 7, 384, 4, 5, 0, 0, 2880},      {3, 7, 384, 4, 5, 0, 1, 2880},      {3, 7, 384, 4, 5, 0, 2, 3332},
        {3, 7, 384, 4, 5, 1, 0, 14348},     {3, 7, 384, 4, 5, 1, 1, 14092},     {3, 7, 384, 4, 5, 1, 2, 14860},
        {256, 100, 1024, 64, 2560, 0, 0, 16785664}, {256, 100, 1024, 64, 2560, 0, 1, 16785664}, {256, 100, 1024, 64, 2560, 0, 2, 16785156},
        {256, 100, 1024, 64, 2560, 1, 0, 19643904}, {256, 100, 1024, 64, 2560, 1, 1, 19684864}, {256, 100, 1024, 64, 2560, 1, 2, 19683840},
    };
    for (const auto &c : parent) check_carve((int)c[0], (int)c[1], (int)c[2], (int)c[3], c[4], c[5] != 0, (int)c[6], c[7]);
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("vec_scoped_layout: ok\n");
    return 0;
}
