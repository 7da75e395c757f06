// fir_split_builds_dump.cpp -- what the host rules answer to the launches of tests/test_fir_split_builds_gpu.py: the geometry of the
// split kernel (periodic_geometry, fir_geometry.cpp), its build (split_build_for), the launch shape (periodic_blocks, the item count
// and item order, the workgroups' item ranges) and, for launches shared among several rate pairs, the deal of workgroups
// (split_deal, fir_split_deal.cpp).  `fir_split_builds_dump <cus>` prints one JSON document:
//   "sweep":  the rates, tap counts and channel counts of fir_geometry_dump.cpp under the default kernel mode: every distinct
//             (NK, WIDE, ROUNDS, groups, images) among the f32 builds they reach, how many rows reach it, and the row with the smallest
//             b (then the smallest a, the fewest taps, the fewest channels, the first in the sweep's order) as
//             `nk= wide= rounds= groups= images= | rows= | taps= ch= in= out= num= den= a= b=`;
//   "nk4":    every swept row of a four-step window;
//   "rows":   one row per request line read from stdin:
//     launch <num> <den> <taps> <channels> <n_streams> <marked streams s,s,..> <abs_out:n_out:streams ...>
//        -> <request> | geo .. | build .. | shape max_blocks= total_items= quads= qpairs= per_group= n= blocks=<per kind> |
//           ranges=<floor(total_items / n)>:<one digit per workgroup: its items beyond that> | marks <stream>=<first item>..<last item>
//           of every slice, each decoded as g<tile group>q<quad>s<stream>b<block>p<pair>
//     geo <num> <den> <taps> <channels>  ->  <request> | geo .. | build ..        (the jobs of the shared launches)
//     deal <total_items:a:groups ...>  ->  <request> | shares=..                  (the jobs of one shared launch, in launch order)
//     note <text>  ->  the line as it is (what the GPU module records beside its launches: chunk lengths, counts from its replay)
// The item order is restated here (item_of) from split_item_record and the counts from make_split_args (fir_split.hip): the kernel
// file cannot be compiled by a host compiler.  tests/test_host_programs.py builds this as plain C++ under ASan + UBSan, feeds it the
// GPU module's requests and compares the output byte for byte with tests/golden/fir_split_builds.json.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "fir_periodic_plan.h"
#include "fir_split_consts.h"

namespace {

struct Shape {
    uint32_t max_blocks, n_streams, pairs, groups, quads, qpairs, per_group, total_items;
};

// make_split_args (fir_split.hip): frames of 8, 12 or 16 channels are cut into quads of two channel pairs, the launch's items are
// slices of (tile group x quad); total_items = max_blocks * n_streams * pairs * groups.
Shape shape_of(const rsmp::PeriodicGeometry& geo, uint32_t n_streams, uint32_t max_blocks) {
    Shape s;
    s.max_blocks = max_blocks;
    s.n_streams = n_streams;
    s.pairs = geo.lp;
    s.quads = geo.cg == 2 && s.pairs >= 4 && s.pairs % 2 == 0 ? s.pairs / 2 : 1u;
    s.qpairs = s.pairs / s.quads;
    s.groups = geo.groups ? geo.groups : 1u;
    s.per_group = max_blocks * n_streams * s.qpairs;
    s.total_items = s.per_group * s.groups * s.quads;
    return s;
}

struct ItemAt {
    uint32_t group, quad, stream, block, pair;
};

// split_item_record (fir_split.hip): slices (tile group x quad); inside a slice streams, blocks of 16 periods, the slice's pairs.
ItemAt item_of(const Shape& g, uint32_t i) {
    const uint32_t slice = i / g.per_group, in_slice = i - slice * g.per_group;
    const uint32_t group = slice / g.quads, quad = slice - group * g.quads;
    const uint32_t per_stream = g.max_blocks * g.qpairs;
    const uint32_t stream = in_slice / per_stream, rem = in_slice - stream * per_stream;
    const uint32_t block = rem / g.qpairs, pair = quad * g.qpairs + (rem - block * g.qpairs);
    return ItemAt{group, quad, stream, block, pair};
}

std::string text_of(const ItemAt& it) {
    char buf[96];
    snprintf(buf, sizeof buf, "g%uq%us%ub%up%u", it.group, it.quad, it.stream, it.block, it.pair);
    return buf;
}

bool launch_row(std::istringstream& in, uint32_t cus, std::string* out) {
    uint64_t num = 0, den = 0;
    uint32_t taps = 0, channels = 0, n_streams = 0;
    std::string marks, kind;
    if (!(in >> num >> den >> taps >> channels >> n_streams >> marks)) return false;
    const rsmp::PeriodicGeometry geo = rsmp::periodic_geometry(num, den, taps, channels);
    if (!geo.ok || geo.mfma != 3) return false;
    const rsmp::SplitChoice c = rsmp::split_build_for(geo, false, rsmp::FirFormat{0, 0, 0, false});
    if (c.error != rsmp::BuildError::kNone) return false;
    uint32_t max_blocks = 0, counted = 0;
    std::string blocks;
    while (in >> kind) {
        unsigned long long abs_out = 0;
        uint32_t n_out = 0, count = 0;
        if (sscanf(kind.c_str(), "%llu:%u:%u", &abs_out, &n_out, &count) != 3) return false;
        const uint32_t b = rsmp::periodic_blocks(geo, abs_out, n_out);
        max_blocks = std::max(max_blocks, b);
        counted += count;
        blocks += (blocks.empty() ? "" : ",") + std::to_string(b);
    }
    if (counted != n_streams || max_blocks == 0) return false;
    const Shape s = shape_of(geo, n_streams, max_blocks);
    const uint32_t n = std::min(s.total_items, cus);   // launch_fir_split: grid = min(total_items, CUs)
    char buf[512];
    snprintf(buf, sizeof buf, " | geo a=%u b=%u den=%u row_len=%u n_tiles=%u groups=%u rounds=%u images=%u cg=%u lp=%u | build nk=%d planes=%d diag=%d wide=%d rounds=%d bits=%d",
             geo.a, geo.b, geo.den, geo.row_len, geo.n_tiles, geo.groups, geo.rounds, geo.images, geo.cg, geo.lp, c.build.nk, c.build.planes, c.build.diag ? 1 : 0,
             c.build.wide, c.build.rounds, c.build.bits);
    *out += buf;
    snprintf(buf, sizeof buf, " | shape max_blocks=%u total_items=%u quads=%u qpairs=%u per_group=%u n=%u blocks=%s | ranges=%u:", s.max_blocks, s.total_items, s.quads,
             s.qpairs, s.per_group, n, blocks.c_str(), s.total_items / n);
    *out += buf;
    // fir_split_body: workgroup wg of n takes the items [wg * total / n, (wg + 1) * total / n)
    for (uint32_t wg = 0; wg < n; ++wg) {
        const uint32_t begin = static_cast<uint32_t>(static_cast<uint64_t>(wg) * s.total_items / n);
        const uint32_t end = static_cast<uint32_t>(static_cast<uint64_t>(wg + 1) * s.total_items / n);
        const uint32_t extra = end - begin - s.total_items / n;
        if (extra > 9) return false;
        *out += static_cast<char>('0' + extra);
    }
    *out += " | marks";
    if (marks != "-") {
        std::istringstream ms(marks);
        std::string tok;
        while (std::getline(ms, tok, ',')) {
            const uint32_t stream = static_cast<uint32_t>(strtoul(tok.c_str(), nullptr, 10));
            if (stream >= n_streams) return false;
            *out += " " + tok + "=";
            const uint32_t per_stream = s.max_blocks * s.qpairs;
            for (uint32_t slice = 0; slice < s.groups * s.quads; ++slice) {
                const uint32_t first = slice * s.per_group + stream * per_stream, last = first + per_stream - 1;
                const ItemAt a = item_of(s, first), z = item_of(s, last);
                if (a.stream != stream || z.stream != stream || last >= s.total_items) return false;
                *out += (slice ? "," : "") + std::to_string(first) + ":" + text_of(a) + ".." + std::to_string(last) + ":" + text_of(z);
            }
        }
    }
    return true;
}

// geo <num> <den> <taps> <channels>: the geometry and the build alone
bool geo_row(std::istringstream& in, std::string* out) {
    uint64_t num = 0, den = 0;
    uint32_t taps = 0, channels = 0;
    if (!(in >> num >> den >> taps >> channels)) return false;
    const rsmp::PeriodicGeometry geo = rsmp::periodic_geometry(num, den, taps, channels);
    if (!geo.ok || geo.mfma != 3) return false;
    const rsmp::SplitChoice c = rsmp::split_build_for(geo, false, rsmp::FirFormat{0, 0, 0, false});
    if (c.error != rsmp::BuildError::kNone) return false;
    char buf[512];
    snprintf(buf, sizeof buf, " | geo a=%u b=%u den=%u row_len=%u n_tiles=%u groups=%u rounds=%u images=%u cg=%u lp=%u | build nk=%d planes=%d diag=%d wide=%d rounds=%d bits=%d",
             geo.a, geo.b, geo.den, geo.row_len, geo.n_tiles, geo.groups, geo.rounds, geo.images, geo.cg, geo.lp, c.build.nk, c.build.planes, c.build.diag ? 1 : 0,
             c.build.wide, c.build.rounds, c.build.bits);
    *out += buf;
    return true;
}

bool deal_row(std::istringstream& in, uint32_t cus, std::string* out) {
    rsmp::DealJob jobs[rsmp::kMaxSplitJobs];
    uint32_t n = 0, share[rsmp::kMaxSplitJobs] = {};
    std::string tok;
    while (in >> tok) {
        if (n == rsmp::kMaxSplitJobs || sscanf(tok.c_str(), "%u:%u:%u", &jobs[n].total_items, &jobs[n].a, &jobs[n].groups) != 3) return false;
        ++n;
    }
    if (n == 0 || !rsmp::split_deal(jobs, n, cus, share)) return false;
    *out += " | shares=";
    for (uint32_t j = 0; j < n; ++j) *out += (j ? "," : "") + std::to_string(share[j]);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const uint32_t cus = argc > 1 ? static_cast<uint32_t>(strtoul(argv[1], nullptr, 10)) : 0u;
    if (cus == 0) {
        fprintf(stderr, "usage: fir_split_builds_dump <cus> < requests\n");
        return 2;
    }
    // ---- the sweep (fir_geometry_dump.cpp's inputs, mode 0)
    static const uint32_t rates[10] = {22050, 16000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 384000};
    static const uint32_t taps_of[4] = {16, 32, 64, 128};
    static const uint32_t channels_of[9] = {1, 2, 3, 4, 6, 8, 12, 16, 17};
    std::vector<std::pair<uint32_t, uint32_t>> pairs;
    for (int i = 0; i < 10; ++i)
        for (int o = 0; o < 10; ++o)
            if (i != o) pairs.emplace_back(rates[i], rates[o]);
    pairs.emplace_back(24000u, 16000u);
    typedef std::tuple<int, int, int, uint32_t, uint32_t> Combination;   // NK, WIDE, ROUNDS, groups, images
    typedef std::tuple<uint32_t, uint32_t, uint32_t, uint32_t> Order;     // b, a, taps, channels
    struct Best { uint32_t rows = 0; Order order; std::string text; };
    std::map<Combination, Best> found;
    std::vector<std::string> nk4;
    for (uint32_t taps : taps_of)
        for (uint32_t ch : channels_of)
            for (const auto& p : pairs) {
                const uint32_t g0 = std::gcd(p.first, p.second);
                const uint32_t num = p.first / g0, den = p.second / g0;
                const rsmp::PeriodicGeometry g = rsmp::periodic_geometry(num, den, taps, ch, true, true);
                if (!g.ok || g.mfma != 3) continue;
                const rsmp::SplitChoice c = rsmp::split_build_for(g, false, rsmp::FirFormat{0, 0, 0, false});
                if (c.error != rsmp::BuildError::kNone || c.build.planes != 2 || c.build.diag || c.build.bits != 0 || c.build.pcm_out) return 1;
                char buf[256];
                snprintf(buf, sizeof buf, "taps=%u ch=%u in=%u out=%u num=%u den=%u a=%u b=%u", taps, ch, p.first, p.second, num, den, g.a, g.b);
                Best& best = found[Combination(c.build.nk, c.build.wide, c.build.rounds, g.groups, g.images)];
                const Order order(g.b, g.a, taps, ch);
                if (best.rows++ == 0 || order < best.order) {
                    best.order = order;
                    best.text = buf;
                }
                if (c.build.nk == 4) nk4.push_back("wide=" + std::to_string(c.build.wide) + " | " + buf);
            }
    // ---- the requests
    std::vector<std::string> rows;
    std::string line;
    char raw[8192];
    while (fgets(raw, sizeof raw, stdin)) {
        line = raw;
        while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string what, row = line;
        in >> what;
        const bool ok = what == "launch" ? launch_row(in, cus, &row) : what == "deal" ? deal_row(in, cus, &row) : what == "geo" ? geo_row(in, &row) : what == "note";
        if (!ok) {
            fprintf(stderr, "fir_split_builds_dump: cannot answer the request `%s`\n", line.c_str());
            return 1;
        }
        rows.push_back(row);
    }
    printf("{\n\"cus\": %u,\n\"sweep\": [\n", cus);
    size_t i = 0;
    for (const auto& kv : found) {
        const Combination& k = kv.first;
        printf("  \"nk=%d wide=%d rounds=%d groups=%u images=%u | rows=%u | %s\"%s\n", std::get<0>(k), std::get<1>(k), std::get<2>(k), std::get<3>(k), std::get<4>(k),
               kv.second.rows, kv.second.text.c_str(), ++i < found.size() ? "," : "");
    }
    printf("],\n\"nk4\": [\n");
    for (i = 0; i < nk4.size(); ++i) printf("  \"%s\"%s\n", nk4[i].c_str(), i + 1 < nk4.size() ? "," : "");
    printf("],\n\"rows\": [\n");
    for (i = 0; i < rows.size(); ++i) printf("  \"%s\"%s\n", rows[i].c_str(), i + 1 < rows.size() ? "," : "");
    printf("]\n}\n");
    return 0;
}
