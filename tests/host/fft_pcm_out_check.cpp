// fft_pcm_out_check.cpp -- fft_choose with PCM output (FftRequest::out_bits), over the requests of fft_launch_cases.h -- those
// tests/golden/fft_launch.json pins: `fft_pcm_out_check <0|1>` (the ordinary / the exact build).  A request that gets the
// pair family gets, with out_bits 16 / 24 / 32, the identical launch (family, build, grid, block, LDS, run arguments: the
// cut of blocks into runs is the f32 twin's); every other request gets kNotSupported; so does a width that is none.
// tests/test_fft_pcm_out_host.py builds it with ASan + UBSan.  Prints the walk's rows, then a summary line.
#include <cstring>

#include "fft_launch.h"
#include "fft_launch_cases.h"

static bool same(const rsmp::FftLaunch& a, const rsmp::FftLaunch& b) {
    bool eq = a.family == b.family && a.pair == b.pair && a.chm == b.chm && a.occ == b.occ && a.bits == b.bits && a.whole_rows == b.whole_rows &&
              a.block == b.block && a.lds == b.lds && a.grant_lds == b.grant_lds && a.n_args == b.n_args;
    for (int i = 0; i < 3; ++i) eq = eq && a.grid[i] == b.grid[i];
    for (int i = 0; i < 6; ++i) eq = eq && a.args[i] == b.args[i];
    return eq;
}

int main(int argc, char** argv) {
    const bool exact = argc > 1 && strcmp(argv[1], "1") == 0;
    long pair = 0, other = 0, bad = 0;
    fft_cases::walk(exact, [&](const fft_cases::Plan& p, const fft_cases::Request& q, int) {
        rsmp::FftShape s{};
        s.fft_in = p.fft_in; s.fft_out = p.fft_out;
        s.n_stages_f = p.n_stages_f; s.n_stages_i = p.n_stages_i;
        for (int i = 0; i < 8; ++i) { s.radix_f[i] = p.radix_f[i]; s.radix_i[i] = p.radix_i[i]; }
        s.n_rc_f = p.n_rc_f; s.n_rc_i = p.n_rc_i;
        s.new_length = p.new_length; s.lds_complex = p.lds_complex;
        s.chirps = true;
        rsmp::FftRequest rq{q.n_streams, q.max_blocks, q.max_channels, q.min_channels, q.pcm_bits, q.exact, q.cus};
        const rsmp::FftLaunch f32 = rsmp::fft_choose(s, rq);
        const bool is_pair = f32.family == rsmp::FftFamily::kPair;
        ++(is_pair ? pair : other);
        fft_cases::Result r;
        r.status = "ok";
        r.kernel = is_pair ? "pair" : "other";
        for (uint32_t out_bits : {16u, 24u, 32u, 8u}) {
            rq.out_bits = out_bits;
            const rsmp::FftLaunch c = rsmp::fft_choose(s, rq);
            const bool good = is_pair && out_bits != 8 ? same(c, f32) : same(c, rsmp::FftLaunch{});
            if (!good) { ++bad; r.status = "invalid"; }
        }
        return r;
    });
    printf("fft_pcm_out_check: %s pair %ld other %ld bad %ld\n", bad == 0 ? "ok" : "FAILED", pair, other, bad);
    return bad == 0 ? 0 : 1;
}
