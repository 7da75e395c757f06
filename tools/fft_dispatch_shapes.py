"""Which kernel, grid, workgroup and LDS size the FFT launches of a build get, as rocprofv3 sees them -- to compare two builds
(RSMP_AMD_LIB selects the library) line for line.  usage (GPU box):
  rocprofv3 --kernel-trace -f csv -d OUT -- python tools/fft_dispatch_shapes.py default
  RSMP_DEBUG=1 RSMP_FFT_WAVE=0 rocprofv3 --kernel-trace -f csv -d OUT0 -- python tools/fft_dispatch_shapes.py wave0
  python tools/fft_dispatch_shapes.py list OUT      (the FFT dispatches of a trace: name | grid | workgroup | LDS, in order)
default: one launch per family at its smallest shape -- pair kernel, the wave kernel's two-channel / channel-pairs / any-channel
builds, the one-buffer kernel -- and bench.py's FFT workload (64 streams x 892 blocks); wave0: the 44.1 <-> 48 kHz workgroup kernel,
its two-channel build, the generic kernel's one-wave workgroups (the switches are read once per process)."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
mode = sys.argv[1]
if mode == "list":
    import csv, glob
    rows = []
    for f in sorted(glob.glob(sys.argv[2] + "/**/*kernel_trace.csv", recursive=True)):
        for r in csv.DictReader(open(f)):
            if "fft_" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), "%s | grid %s %s %s | workgroup %s %s %s | lds %s" % (
                    r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"],
                    r["Workgroup_Size_Z"], " ".join(r[k] for k in r if "LDS" in k.upper()))))
    for _, line in sorted(rows):
        print(line)
    sys.exit(0)
import numpy as np, torch
import resampler_amd as ra
from resampler_amd import synth
R = [22050, 16000, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 384000]
dev = torch.device("cuda:0")
shapes = {"default": [(44100, 48000, 2, 4), (44100, 48000, 2, 3), (44100, 48000, 4, 7), (44100, 48000, 3, 7), (16000, 384000, 1, 3)],
          "wave0": [(44100, 48000, 1, 9), (44100, 48000, 2, 9), (96000, 48000, 1, 9)]}[mode]
for a, b, ch, blocks in shapes:
    g = ra.ResamplerFft.new(ch, ra.SampleRate(R.index(a)), ra.SampleRate(R.index(b)))
    n_in, n_out = g.chunk_size_input(), g.chunk_size_output()
    d_in = torch.from_numpy(synth.fast_noise(blocks * n_in, seed=5)).to(dev)
    d_out = torch.zeros(blocks * n_out, device=dev)
    torch.cuda.synchronize()
    g.resample_bulk_device(d_in, d_out, blocks)
    torch.cuda.synchronize()
    print("ran", a, b, ch, blocks, float(d_out.abs().max()))
if mode == "default":
    S, blocks = 64, 892
    hs = [ra.ResamplerFft.new(2, ra.SampleRate.Hz44100, ra.SampleRate.Hz48000) for _ in range(S)]
    n_in, n_out = hs[0].chunk_size_input(), hs[0].chunk_size_output()
    base = torch.from_numpy(synth.sweep(blocks * n_in // 2, 2, 44100.0)).to(dev)
    d_in = [base for _ in range(S)]
    d_out = [torch.empty(blocks * n_out, device=dev) for _ in range(S)]
    batch = ra.FftBatch(hs)
    batch.bind(d_in, d_out, [blocks] * S)
    torch.cuda.synchronize()
    batch.resample_bulk_device(ra.torch_stream())
    torch.cuda.synchronize()
    print("ran bench shape", S, blocks)
