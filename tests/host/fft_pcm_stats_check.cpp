// fft_pcm_stats_check.cpp -- fft_choose with the statistics flag (FftRequest::pcm_stats), over the requests of fft_launch_cases.h --
// those tests/golden/fft_launch.json pins: `fft_pcm_stats_check <0|1>` (the ordinary / the exact build).  With out_bits 16 / 24 / 32
// the flag changes nothing of the launch -- family, build, grid, block, LDS, run arguments: every field of FftLaunch but
// pcm_stats, which is set exactly where the launch is the pair kernel's --; with out_bits 0 the flag is kNotSupported whatever the
// request would get without it.  tests/test_fft_pcm_stats.py builds it with ASan + UBSan.  Prints the walk's rows, then a summary.
#include <cstring>

#include "fft_launch.h"
#include "fft_launch_cases.h"

// every field but the flag
static bool same(const rsmp::FftLaunch& a, const rsmp::FftLaunch& b) {
    bool eq = a.family == b.family && a.pair == b.pair && a.chm == b.chm && a.occ == b.occ && a.bits == b.bits && a.whole_rows == b.whole_rows &&
              a.block == b.block && a.lds == b.lds && a.grant_lds == b.grant_lds && a.n_args == b.n_args;
    for (int i = 0; i < 3; ++i) eq = eq && a.grid[i] == b.grid[i];
    for (int i = 0; i < 6; ++i) eq = eq && a.args[i] == b.args[i];
    return eq;
}

int main(int argc, char** argv) {
    const bool exact = argc > 1 && strcmp(argv[1], "1") == 0;
    long counting = 0, other = 0, bad = 0;
    fft_cases::walk(exact, [&](const fft_cases::Plan& p, const fft_cases::Request& q, int) {
        rsmp::FftShape s{};
        s.fft_in = p.fft_in; s.fft_out = p.fft_out;
        s.n_stages_f = p.n_stages_f; s.n_stages_i = p.n_stages_i;
        for (int i = 0; i < 8; ++i) { s.radix_f[i] = p.radix_f[i]; s.radix_i[i] = p.radix_i[i]; }
        s.n_rc_f = p.n_rc_f; s.n_rc_i = p.n_rc_i;
        s.new_length = p.new_length; s.lds_complex = p.lds_complex;
        s.chirps = true;
        rsmp::FftRequest rq{q.n_streams, q.max_blocks, q.max_channels, q.min_channels, q.pcm_bits, q.exact, q.cus};
        fft_cases::Result r;
        r.status = "ok";
        r.kernel = "other";
        auto fail = [&] { ++bad; r.status = "invalid"; };
        // out_bits == 0: nothing to count
        rq.out_bits = 0;
        rq.pcm_stats = true;
        const rsmp::FftLaunch none = rsmp::fft_choose(s, rq);
        if (!same(none, rsmp::FftLaunch{}) || none.family != rsmp::FftFamily::kNotSupported || none.pcm_stats) fail();
        bool is_pair = false;
        for (uint32_t out_bits : {16u, 24u, 32u}) {
            rq.out_bits = out_bits;
            rq.pcm_stats = false;
            const rsmp::FftLaunch off = rsmp::fft_choose(s, rq);
            rq.pcm_stats = true;
            const rsmp::FftLaunch on = rsmp::fft_choose(s, rq);
            is_pair = off.family == rsmp::FftFamily::kPair;
            if (!same(on, off) || off.pcm_stats || on.pcm_stats != is_pair) fail();
            if (!is_pair && off.family != rsmp::FftFamily::kNotSupported) fail();
        }
        if (is_pair) r.kernel = "pair";
        ++(is_pair ? counting : other);
        return r;
    });
    printf("fft_pcm_stats_check: %s pair %ld other %ld bad %ld\n", bad == 0 ? "ok" : "FAILED", counting, other, bad);
    return bad == 0 ? 0 : 1;
}
