// fft_launch_dump.cpp -- every decision of fft_launch.cpp for the requests of fft_launch_cases.h, as text: `fft_launch_dump
// <0|1>` (the ordinary / the exact build).  tests/test_host_programs.py builds it with ASan + UBSan, runs it once per
// setting of the debug switches (they are read once per process) and compares with tests/golden/fft_launch.json.
#include <cstring>

#include "fft_launch.h"
#include "fft_launch_cases.h"

static const char* kFamily[] = {"pair", "wave", "ct", "ct2", "generic", "big"};

int main(int argc, char** argv) {
    const bool exact = argc > 1 && strcmp(argv[1], "1") == 0;
    fft_cases::walk(exact, [](const fft_cases::Plan& p, const fft_cases::Request& q, int occ) {
        rsmp::FftShape s{};
        s.fft_in = p.fft_in; s.fft_out = p.fft_out;
        s.n_stages_f = p.n_stages_f; s.n_stages_i = p.n_stages_i;
        for (int i = 0; i < 8; ++i) { s.radix_f[i] = p.radix_f[i]; s.radix_i[i] = p.radix_i[i]; }
        s.n_rc_f = p.n_rc_f; s.n_rc_i = p.n_rc_i;
        s.new_length = p.new_length; s.lds_complex = p.lds_complex;
        s.chirps = true;
        const rsmp::FftRequest rq{q.n_streams, q.max_blocks, q.max_channels, q.min_channels, q.pcm_bits, q.exact, q.cus};
        rsmp::FftLaunch c = rsmp::fft_choose(s, rq);
        fft_cases::Result r;
        if (c.family == rsmp::FftFamily::kInvalid) r.status = "invalid";
        if (c.family >= rsmp::FftFamily::kNotSupported) return r;
        r.status = "ok";
        if (c.family != rsmp::FftFamily::kPair && c.family != rsmp::FftFamily::kWave) {
            r.asked_occupancy = true;
            rsmp::fft_choose_run(&c, rq, occ);
        }
        char name[96];
        snprintf(name, sizeof name, "%s pair=%d chm=%d occ=%d bits=%d threads=%u", kFamily[static_cast<int>(c.family)], c.pair, c.chm, c.occ,
                 c.bits, c.family == rsmp::FftFamily::kGeneric ? c.block : 0u);
        r.kernel = name;
        for (int i = 0; i < 3; ++i) r.grid[i] = c.grid[i];
        r.block = c.block;
        r.lds = c.lds;
        r.grant = c.grant_lds;
        r.args.assign(c.args, c.args + c.n_args);
        return r;
    });
    return 0;
}
