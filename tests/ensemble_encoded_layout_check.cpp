// Stand-alone check of csrc/ensemble_encoded_layout.h (no HIP, no GPU): the scratch carve of
// mir_block_ensemble_search_scopes_encoded.  tests/test_ensemble_encoded_layout.py builds it with the host compiler and the
// address and undefined-behaviour sanitizers, and runs it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "ensemble_encoded_layout.h"

using namespace mir;

static int failures = 0;
static long carved = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);       \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

static size_t up(size_t x) { return (x + 255) / 256 * 256; }

using Spans = std::vector<std::pair<size_t, size_t>>;

static void check_disjoint(Spans spans, size_t end) {  // whatever the order they were carved in: sort the (begin, end) pairs and compare neighbours
    std::sort(spans.begin(), spans.end());
    for (size_t i = 0; i + 1 < spans.size(); ++i) CHECK(spans[i].second <= spans[i + 1].first);
    for (const auto &sp : spans) CHECK(sp.second <= end);
}

// what must hold of every carve that succeeds: the layout is rebuilt here array by array, in the documented order
static void check_layout(const EnsembleEncodedShape &es, const EnsembleEncodedLayout &l) {
    const EnsembleScopesShape &s = es.base;
    const size_t b = (size_t)s.b, cap = (size_t)s.cap, listed = (size_t)s.listed;
    Spans spans;
    size_t o = 0;
    auto next = [&](size_t at, size_t bytes) {  // the array at `at` is the next one: it starts where the last one ended, rounded up
        CHECK(at == o);
        CHECK(at % 256 == 0);
        spans.push_back({at, at + bytes});
        o = up(at + bytes);
    };
    next(l.scope_ptr, (b + 1) * 4);
    next(l.refs, b * s.ref_bytes);
    for (int i = 0; i < s.n_legs; ++i) {
        const EnsembleScopesLegShape &g = s.leg[i];
        const EnsembleScopesLegLayout &at = l.leg[i];
        if (g.kind == kScopesLegKeyword) {
            next(at.terms, ((size_t)g.terms + 1) * 4);
            next(at.q_ptr, (b + 1) * 4);
            next(at.scopes, b * s.scope_bytes);
        } else if (es.leg_mask >> i & 1) {
            CHECK(at.q == l.q_enc);  // every masked leg reads the one array the device writes
        } else if (g.q_of >= 0) {
            CHECK(at.q == l.leg[g.q_of].q);
        } else {
            next(at.q, b * (size_t)g.d * 8);
        }
    }
    CHECK(l.in_bytes == o);  // the upload span: contiguous from 0, no query bytes of a masked leg
    const size_t in_arrays = spans.size();
    next(l.q_enc, b * 384 * 8);
    CHECK(l.q_enc >= l.in_bytes);  // the masked q lies outside the upload span ...
    if (!es.want_emb) next(l.emb, b * 384 * 4);
    for (int i = 0; i < s.n_legs; ++i) {
        if (s.leg[i].kind != kScopesLegVector) continue;
        next(l.leg[i].table, listed * s.desc_bytes);
        if (s.leg[i].expanded) next(l.leg[i].fan_table, listed * s.fan_bytes);
        else CHECK(l.leg[i].fan_table == 0);
    }
    for (int i = 0; i < s.n_legs; ++i) {
        const EnsembleScopesLegShape &g = s.leg[i];
        if (g.kind != kScopesLegVector) continue;
        next(l.leg[i].l_doc, b * (size_t)g.k * 4);
        next(l.leg[i].l_chunk, b * (size_t)g.k * 8);
        next(l.leg[i].l_count, b * 4);
    }
    const size_t down = o;
    next(l.f_doc, b * cap * 4);
    next(l.f_chunk, b * cap * 8);
    next(l.f_score, b * cap * 8);
    next(l.f_origin, b * cap * 4);
    next(l.f_count, b * 4);
    if (es.want_emb) next(l.emb, b * 384 * 4);  // behind f_count
    CHECK(l.f_doc == down && l.out_bytes == o - down);
    CHECK(l.keyword == o);
    const size_t down_end = l.f_doc + l.out_bytes;
    CHECK(l.q_enc + b * 384 * 8 <= l.f_doc);  // ... and outside the download span
    const bool emb_in_download = l.emb >= l.f_doc && l.emb + b * 384 * 4 <= down_end;
    const bool emb_outside = l.emb >= l.in_bytes && l.emb + b * 384 * 4 <= l.f_doc;
    CHECK(emb_in_download == es.want_emb);  // emb rides in the download exactly when it is wanted
    CHECK(es.want_emb || emb_outside);      // otherwise it is device-only: in neither span
    for (size_t i = 0; i < in_arrays; ++i) CHECK(spans[i].second <= l.in_bytes);
    CHECK(l.in_bytes <= l.keyword && down_end <= l.keyword);  // every span lies inside need
    check_disjoint(spans, l.keyword);
    ++carved;
}

static EnsembleEncodedCarve carve(const EnsembleEncodedShape &s, EnsembleEncodedLayout *l) {
    const EnsembleEncodedCarve rc = ensemble_encoded_carve(s, l);
    if (rc == kEncodedOk) check_layout(s, *l);
    return rc;
}

static EnsembleScopesLegShape vec(int64_t k, int64_t d, bool expanded, int32_t q_of = -1) { return {kScopesLegVector, k, d, 0, expanded, q_of}; }
static EnsembleScopesLegShape kwd(int64_t k, int64_t terms) { return {kScopesLegKeyword, k, 0, terms, false, -1}; }
static EnsembleEncodedShape shape(int64_t b, int64_t cap, int64_t listed, std::vector<EnsembleScopesLegShape> legs, uint32_t mask, bool want_emb) {
    EnsembleEncodedShape es{};
    EnsembleScopesShape &s = es.base;
    s.b = b; s.cap = cap; s.listed = listed; s.n_legs = (int32_t)legs.size();
    for (size_t i = 0; i < legs.size() && i < (size_t)kRrfMaxLists; ++i) s.leg[i] = legs[i];
    s.desc_bytes = 32; s.fan_bytes = 32; s.scope_bytes = 56; s.ref_bytes = sizeof(EnsembleScopeRef);
    es.leg_mask = mask; es.want_emb = want_emb;
    return es;
}

int main() {
    EnsembleEncodedLayout l;
    // the sweep: one to four legs - 1 to 3 vector legs, the keyword leg at every place or absent - the mask on one, two or three
    // vector legs, b, embeddings wanted and not wanted.  A vector leg outside the mask is the multimodal one (d = 64).
    const int64_t bs[] = {1, 2, 255, 256, 257};
    long want = 0;
    for (int slots = 1; slots <= 3; ++slots)
        for (int kw = -1; kw <= slots; ++kw)
            for (int vmask = 1; vmask < (1 << slots); ++vmask)  // which VECTOR legs are masked (by slot)
                for (int emb = 0; emb < 2; ++emb)
                    for (int64_t b : bs) {
                        std::vector<EnsembleScopesLegShape> legs;
                        const int n_legs = slots + (kw >= 0 ? 1 : 0);
                        uint32_t mask = 0;
                        int first = -1, v = 0;
                        for (int i = 0; i < n_legs; ++i) {
                            if (i == kw) { legs.push_back(kwd(7, 3 * b + 1)); continue; }
                            const bool masked = vmask >> v & 1, expanded = v != 0;
                            if (masked) {
                                legs.push_back(vec(7, 384, expanded, first));
                                if (first < 0) first = i;
                                mask |= 1u << i;
                            } else {
                                legs.push_back(vec(7, 64, expanded));
                            }
                            ++v;
                        }
                        CHECK(carve(shape(b, 7 * n_legs, 10 * b, legs, mask, emb != 0), &l) == kEncodedOk);
                        ++want;
                    }
    CHECK(carved == want);
    // exact numbers of one small carve: b = 2, cap = 7, 5 documents; a masked leg (k 3, expanded), a keyword leg (k 2, 6 terms),
    // a host leg (k 1, d 4), a second masked leg (k 1); the embeddings wanted
    CHECK(carve(shape(2, 7, 5, {vec(3, 384, true), kwd(2, 6), vec(1, 4, false), vec(1, 384, false, 0)}, 0x9, true), &l) == kEncodedOk);
    CHECK(l.scope_ptr == 0 && l.refs == 256 && l.leg[1].terms == 512 && l.leg[1].q_ptr == 768 && l.leg[1].scopes == 1024 && l.leg[2].q == 1280);
    CHECK(l.in_bytes == 1536 && l.q_enc == 1536 && l.leg[0].q == 1536 && l.leg[3].q == 1536);  // 2 x 384 x 8 = 6144 bytes
    CHECK(l.leg[0].table == 7680 && l.leg[0].fan_table == 7936 && l.leg[2].table == 8192 && l.leg[3].table == 8448);
    CHECK(l.leg[0].l_doc == 8704 && l.leg[3].l_count == 10752 && l.f_doc == 11008 && l.f_count == 12032 && l.emb == 12288);
    CHECK(l.out_bytes == 1280 + 3072 && l.keyword == 15360);
    // ... and not wanted: emb moves in front of the tables, the download span is the parent's
    CHECK(carve(shape(2, 7, 5, {vec(3, 384, true), kwd(2, 6), vec(1, 4, false), vec(1, 384, false, 0)}, 0x9, false), &l) == kEncodedOk);
    CHECK(l.q_enc == 1536 && l.emb == 7680 && l.leg[0].table == 10752 && l.out_bytes == 1280 && l.keyword == l.f_count + 256);
    // two host legs outside the mask still share their upload
    CHECK(carve(shape(4, 21, 4, {vec(7, 64, false), vec(7, 384, false), vec(7, 64, false, 0)}, 0x2, true), &l) == kEncodedOk);
    CHECK(l.leg[2].q == l.leg[0].q && l.leg[1].q == l.q_enc && l.leg[0].q < l.in_bytes);
    // the timing tool's shape
    CHECK(carve(shape(256, 28, 2560, {vec(7, 384, false), kwd(7, 1024), vec(7, 1024, true), vec(7, 384, true, 0)}, 0x9, true), &l) == kEncodedOk);
    // malformed masks and shapes leave the layout as it was
    const EnsembleEncodedLayout before = l;
    CHECK(carve(shape(4, 14, 0, {vec(7, 384, false), kwd(7, 1)}, 0x0, true), &l) == kEncodedBadMask);                 // empty
    CHECK(carve(shape(4, 14, 0, {vec(7, 384, false), kwd(7, 1)}, 0x2, true), &l) == kEncodedBadMask);                 // the keyword leg
    CHECK(carve(shape(4, 14, 0, {vec(7, 384, false), kwd(7, 1)}, 0x3, true), &l) == kEncodedBadMask);
    CHECK(carve(shape(4, 14, 0, {vec(7, 384, false), kwd(7, 1)}, 0x4, true), &l) == kEncodedBadMask);                 // at n_legs
    CHECK(carve(shape(4, 14, 0, {vec(7, 384, false), kwd(7, 1)}, 0x5, true), &l) == kEncodedBadMask);
    CHECK(carve(shape(4, 14, 0, {vec(7, 384, false), kwd(7, 1)}, 0x80000001u, true), &l) == kEncodedBadMask);         // beyond it
    CHECK(carve(shape(4, 7, 0, {vec(7, 64, false)}, 0x1, true), &l) == kEncodedBadMask);                              // a masked leg at d = 64
    CHECK(carve(shape(4, 14, 0, {vec(7, 384, false), vec(7, 383, false)}, 0x2, true), &l) == kEncodedBadMask);
    CHECK(carve(shape(4, 14, 0, {vec(7, 384, false), vec(7, 384, false)}, 0x3, true), &l) == kEncodedBadShape);       // masked legs that do not share
    CHECK(carve(shape(4, 14, 0, {vec(7, 384, false), vec(7, 384, false, 0)}, 0x1, true), &l) == kEncodedBadShape);    // a host leg on the device's array
    CHECK(carve(shape(4, 14, 0, {vec(7, 384, false), vec(7, 384, false, 0)}, 0x2, true), &l) == kEncodedBadShape);    // a masked leg on a host leg's
    CHECK(carve(shape(4, 7, 0, {}, 0x1, true), &l) == kEncodedBadShape);
    CHECK(carve(shape(-1, 7, 0, {vec(7, 384, false)}, 0x1, true), &l) == kEncodedBadShape);
    CHECK(carve(shape(4, 7, -1, {vec(7, 384, false)}, 0x1, true), &l) == kEncodedBadShape);
    CHECK(carve(shape(4, 7, 0, {vec(0, 384, false)}, 0x1, true), &l) == kEncodedBadShape);
    CHECK(carve(shape(4, 6, 0, {vec(7, 384, false)}, 0x1, true), &l) == kEncodedBadShape);  // cap < sum k
    CHECK(carve(shape(4, 28, 0, {vec(7, 384, false), vec(7, 384, false, 0), vec(7, 384, false, 0), vec(7, 384, false, 0)}, 0xf, true), &l) == kEncodedBadShape);  // four slots
    CHECK(carve(shape(4, 14, 0, {kwd(7, 1), kwd(7, 1)}, 0x1, true), &l) == kEncodedBadShape);
    CHECK(carve(shape(4, 513, 4, {vec(128, 384, false), kwd(129, 4), vec(128, 8, true), vec(128, 384, true, 0)}, 0x9, true), &l) == kEncodedTooManyItems);
    // sizes that would leave size_t's comfortable range are refused, not wrapped: an array of 2^40 bytes or more
    CHECK(carve(shape((int64_t)1 << 31, 7, 0, {vec(7, 384, false)}, 0x1, true), &l) == kEncodedTooLarge);
    CHECK(carve(shape((int64_t)1 << 29, 7, 0, {vec(7, 384, false)}, 0x1, true), &l) == kEncodedTooLarge);  // q: 2^29 x 3072 bytes
    CHECK(carve(shape(INT32_MAX, 512, 0, {vec(7, 384, false)}, 0x1, false), &l) == kEncodedTooLarge);
    CHECK(carve(shape(4, 7, (int64_t)1 << 31, {vec(7, 384, true)}, 0x1, true), &l) == kEncodedTooLarge);
    CHECK(carve(shape(4, 14, 0, {vec(7, 384, false), kwd(7, (int64_t)1 << 40)}, 0x1, true), &l) == kEncodedTooLarge);
    CHECK(l.keyword == before.keyword && l.f_doc == before.f_doc && l.q_enc == before.q_enc && l.emb == before.emb);
    // a large call that is still accepted stays far inside 2^63
    CHECK(carve(shape(1 << 20, 512, INT32_MAX, {vec(128, 1024, true), kwd(128, INT32_MAX), vec(128, 384, true), vec(128, 384, true, 2)}, 0xc, true), &l) == kEncodedOk);
    CHECK(l.keyword > l.emb && l.keyword < ((size_t)1 << 48));
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("ensemble_encoded_layout: ok (%ld carves)\n", carved);
    return 0;
}
