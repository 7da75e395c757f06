// pcm_batch_plan_check.cpp -- stand-alone check of the batched PCM converters' plan (resampler_amd/csrc/pcm_batch_plan.h), the very
// functions the kernels run: the prefix of tile counts, the search that names a tile's stream, the walk from one tile to a later
// one, and the deal of tiles to the workgroups of a grid.  Built by tests/test_pcm_batch.py with g++ under ASan + UBSan.
//   pcm_batch_plan_check   ->   "pcm_batch_plan_check: ok sets <n> tiles <n> bad 0"
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pcm_batch_plan.h"

namespace {

using namespace rsmp;

uint64_t g_rng = 0x243F6A8885A308D3ull;
uint64_t rnd() {   // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

long g_bad = 0;
unsigned long long g_tiles = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (g_bad++ < 20) {                            \
                std::printf("FAIL %s: ", #cond);           \
                std::printf(__VA_ARGS__);                  \
                std::printf("\n");                         \
            }                                              \
        }                                                  \
    } while (0)

// One tile of the launch checked against its stream: the search, and the values it covers.
void check_tile(const std::vector<uint64_t>& lens, const std::vector<uint32_t>& prefix, uint32_t tile, uint32_t want_stream) {
    const uint32_t n = static_cast<uint32_t>(lens.size());
    const uint32_t s = pcm_batch_find_stream(prefix.data(), n, tile);
    CHECK(s == want_stream, "tile %u: stream %u, want %u", tile, s, want_stream);
    if (s >= n) return;
    CHECK(lens[s] != 0, "tile %u: empty stream %u", tile, s);
    CHECK(prefix[s] <= tile && tile < prefix[s + 1], "tile %u outside stream %u's [%u, %u)", tile, s, prefix[s], prefix[s + 1]);
    const uint64_t base = static_cast<uint64_t>(tile - prefix[s]) * kPcmBatchTile;
    CHECK(base % 4 == 0 && base < lens[s], "tile %u: base %llu of %llu", tile, (unsigned long long)base, (unsigned long long)lens[s]);
}

// Every tile of a set of streams: the tiles partition every stream's values exactly once, none straddles two streams, the prefix is
// monotone, the search names the right stream, the walk from any earlier tile does too.
void check_set(const std::vector<uint64_t>& lens, bool exhaustive) {
    const uint32_t n = static_cast<uint32_t>(lens.size());
    std::vector<uint32_t> prefix(n + 1, 0xDEADBEEFu);
    const bool ok = pcm_batch_prefix(lens.data(), n, prefix.data());
    CHECK(ok, "a batch that fits was refused");
    if (!ok) return;
    CHECK(prefix[0] == 0, "prefix[0] = %u", prefix[0]);
    uint64_t total = 0;
    for (uint32_t s = 0; s < n; ++s) {
        CHECK(prefix[s] == total, "prefix[%u] = %u, want %llu", s, prefix[s], (unsigned long long)total);
        CHECK(prefix[s + 1] >= prefix[s], "prefix not monotone at %u", s);
        const uint64_t t = pcm_batch_stream_tiles(lens[s]);
        CHECK(t * kPcmBatchTile >= lens[s] && (t == 0 || (t - 1) * kPcmBatchTile < lens[s]), "stream %u: %llu tiles for %llu values", s,
              (unsigned long long)t, (unsigned long long)lens[s]);
        CHECK((lens[s] == 0) == (t == 0), "stream %u: empty <-> no tile", s);
        total += t;
    }
    CHECK(prefix[n] == total, "prefix[n] = %u, want %llu", prefix[n], (unsigned long long)total);
    // the values: tile j of stream s covers [j T, min((j + 1) T, len)) -- summed over the stream's tiles that is len, each value once
    for (uint32_t s = 0; s < n; ++s) {
        const uint64_t t = prefix[s + 1] - prefix[s];
        if (t == 0) continue;
        const uint64_t covered = (t - 1) * kPcmBatchTile + (lens[s] - (t - 1) * kPcmBatchTile);
        CHECK(covered == lens[s] && lens[s] - (t - 1) * kPcmBatchTile <= kPcmBatchTile, "stream %u: covered %llu of %llu", s, (unsigned long long)covered,
              (unsigned long long)lens[s]);
    }
    // the search: every tile (exhaustive), or a stream's first, second and last tiles and seeded ones
    uint32_t walk = 0;   // the walk, started once and carried over all the tiles in order
    bool walking = false;
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t p0 = prefix[s], p1 = prefix[s + 1];
        if (p0 == p1) continue;
        std::vector<uint32_t> probe;
        if (exhaustive || p1 - p0 <= 64) {
            for (uint32_t t = p0; t < p1; ++t) probe.push_back(t);
        } else {
            probe = {p0, p0 + 1, p1 - 2, p1 - 1};
            for (int k = 0; k < 64; ++k) probe.push_back(p0 + static_cast<uint32_t>(rnd() % (p1 - p0)));
        }
        for (uint32_t t : probe) {
            check_tile(lens, prefix, t, s);
            ++g_tiles;
        }
        // (the walk from the last stream that had a tile crosses every empty stream between the two)
        if (!walking) {
            walk = pcm_batch_find_stream(prefix.data(), n, p0);
            walking = true;
        }
        walk = pcm_batch_walk(prefix.data(), walk, p0);
        CHECK(walk == s, "walk to tile %u: stream %u, want %u", p0, walk, s);
        walk = pcm_batch_walk(prefix.data(), walk, p1 - 1);
        CHECK(walk == s, "walk to tile %u: stream %u, want %u", p1 - 1, walk, s);
    }
    // the deal: on grids of several sizes, both orders, every tile goes to exactly one workgroup
    const uint32_t tiles = prefix[n];
    if (tiles == 0 || tiles > (1u << 22)) return;
    for (uint32_t cus : {1u, 3u, 64u, 256u, 304u}) {
        const uint32_t G = pcm_batch_grid(tiles, cus);
        CHECK(G >= 1 && G <= tiles && G <= cus * kPcmBatchWgPerCu, "grid %u for %u tiles, %u CUs", G, tiles, cus);
        for (uint32_t order : {static_cast<uint32_t>(kPcmBatchContiguous), static_cast<uint32_t>(kPcmBatchStrided)}) {
            std::vector<uint8_t> seen(tiles, 0);
            uint64_t dealt = 0;
            for (uint32_t w = 0; w < G; ++w) {
                const PcmBatchDeal d = pcm_batch_deal(order, w, G, tiles);
                uint64_t t = d.first;
                for (uint32_t i = 0; i < d.count; ++i, t += d.step) {
                    CHECK(t < tiles, "order %u: workgroup %u of %u deals tile %llu of %u", order, w, G, (unsigned long long)t, tiles);
                    if (t < tiles) ++seen[t];
                    ++dealt;
                }
            }
            CHECK(dealt == tiles, "order %u, grid %u: %llu tiles dealt of %u", order, G, (unsigned long long)dealt, tiles);
            for (uint32_t t = 0; t < tiles; ++t)
                if (seen[t] != 1) {
                    CHECK(false, "order %u, grid %u: tile %u dealt %u times", order, G, t, seen[t]);
                    break;
                }
        }
    }
}

}  // namespace

int main() {
    const uint64_t T = kPcmBatchTile;
    static_assert(kPcmBatchTile % 4 == 0, "T is a multiple of 4");
    const uint64_t special[] = {0, 1, 2, 3, 4, 5, T - 1, T, T + 1, 2 * T, 2 * T + 3, 0, 0, 0};
    long sets = 0;
    // the edge lengths alone, in order and reversed, with empty streams at both ends
    {
        std::vector<uint64_t> lens(std::begin(special), std::end(special));
        check_set(lens, true);
        std::vector<uint64_t> rev(lens.rbegin(), lens.rend());
        check_set(rev, true);
        check_set(std::vector<uint64_t>{0, 0, 0, 1}, true);
        check_set(std::vector<uint64_t>{1, 0, 0, 0}, true);
        check_set(std::vector<uint64_t>{0, 0, 0}, true);
        check_set(std::vector<uint64_t>{T}, true);
        check_set(std::vector<uint64_t>{}, true);
        sets += 7;
    }
    // seeded sets: lengths from the edge list, runs of empty streams, and lengths up to a few tiles
    for (int set = 0; set < 200; ++set) {
        const size_t n = 1 + static_cast<size_t>(rnd() % 300);
        std::vector<uint64_t> lens;
        while (lens.size() < n) {
            const uint64_t kind = rnd() % 8;
            if (kind == 0) {   // a run of empty streams
                for (uint64_t k = 1 + rnd() % 6; k > 0 && lens.size() < n; --k) lens.push_back(0);
            } else if (kind <= 3) {
                lens.push_back(special[rnd() % (sizeof special / sizeof special[0])]);
            } else {
                lens.push_back(rnd() % (5 * T));
            }
        }
        check_set(lens, true);
        ++sets;
    }
    // one stream of 2^40 values among short and empty ones (its 2^28 tiles are probed, not walked one by one)
    {
        std::vector<uint64_t> lens = {3, 0, 0, T + 1, 1ull << 40, 0, 5, (1ull << 40) + 1, 0, T - 1, 0};
        check_set(lens, false);
        ++sets;
    }
    // a batch whose tiles do not fit 32 bits is refused; the largest that fits is not
    {
        std::vector<uint32_t> prefix(4);
        const uint64_t most = 0xFFFFFFFFull * T;   // 2^32 - 1 tiles
        const uint64_t a[] = {most, 1, 0}, b[] = {most, 0, 0}, c[] = {most + 1, 0, 0}, d[] = {most - T, T, 1}, e[] = {~0ull, 0, 0}, f[] = {most / 2 + T, most / 2 + T, 5};
        CHECK(!pcm_batch_prefix(a, 3, prefix.data()), "2^32 tiles accepted");
        CHECK(pcm_batch_prefix(b, 3, prefix.data()) && prefix[3] == 0xFFFFFFFFu, "2^32 - 1 tiles refused");
        CHECK(!pcm_batch_prefix(c, 3, prefix.data()), "2^32 tiles in one stream accepted");
        CHECK(!pcm_batch_prefix(d, 3, prefix.data()), "2^32 tiles over three streams accepted");
        CHECK(!pcm_batch_prefix(e, 3, prefix.data()), "a stream of 2^64 - 1 values accepted");
        CHECK(!pcm_batch_prefix(f, 3, prefix.data()), "two halves above 2^32 tiles accepted");
        // ... and in the largest batch the search still names the last tile's stream
        const uint64_t g[] = {most - T, 0, T};
        CHECK(pcm_batch_prefix(g, 3, prefix.data()), "2^32 - 1 tiles over two streams refused");
        CHECK(pcm_batch_find_stream(prefix.data(), 3, 0xFFFFFFFEu) == 2 && pcm_batch_find_stream(prefix.data(), 3, 0xFFFFFFFDu) == 0, "search at the 32-bit edge");
        const PcmBatchDeal last = pcm_batch_deal(kPcmBatchContiguous, 1023, 1024, 0xFFFFFFFFu);
        CHECK(static_cast<uint64_t>(last.first) + last.count == 0xFFFFFFFFull, "the last workgroup's range ends at the last tile");
        ++sets;
    }
    std::printf("pcm_batch_plan_check: %s sets %ld tiles %llu bad %ld\n", g_bad ? "FAILED" : "ok", sets, g_tiles, g_bad);
    return g_bad ? 1 : 0;
}
