"""What the hardware gives per byte in flight: `nt` streaming reads of a 1-GiB buffer (far larger than the Infinity Cache) with
16 / 32 / 48 / 64 / 96 / 128 / 256 KB outstanding per CU (bprx_probe_stream_read_nt_shape: one 1024-thread workgroup per CU,
1 .. 16 loads of 16 B in flight per lane; and the same bytes as two 512-thread workgroups per CU where that shape exists).
Best of 5 timed launches after 2 warm-ups, events on the launch stream.
    python scripts/nt_inflight_sweep.py > profiles/nt_inflight_sweep.txt"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fashionvisualexpl_recommend_amd import _ffi

L = _ffi.lib()
dev = torch.device("cuda:0")
ncu = torch.cuda.get_device_properties(0).multi_processor_count
nbytes = 1 << 30
buf = torch.ones(nbytes // 4, dtype=torch.float32, device=dev)
sink = torch.zeros(4096, dtype=torch.float32, device=dev)
st = torch.cuda.Stream()


def rate(wg, thr, u):
    best = 0.0
    with torch.cuda.stream(st):
        for it in range(7):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            got = L.bprx_probe_stream_read_nt_shape(C.c_void_p(buf.data_ptr()), nbytes, wg, thr, u, C.c_void_p(sink.data_ptr()),
                                                    C.c_void_p(st.cuda_stream))
            b.record(st)
            b.synchronize()
            if got < 0:
                raise RuntimeError("bprx_probe_stream_read_nt_shape(%d, %d, %d) failed: %d" % (wg, thr, u, got))
            if it >= 2:
                best = max(best, got / (a.elapsed_time(b) * 1e-3) / 1e9)
    return best


print("# %s, %d CUs; nt loads over 1 GiB; GB/s, best of 5" % (torch.cuda.get_device_name(0), ncu))
print("# KB in flight per CU | workgroups x threads x loads per lane | GB/s")
for u in (1, 2, 3, 4, 6, 8, 16):
    kb = 1024 * u * 16 // 1024
    print("%4d KB  %4d x 1024 x %2d  %8.1f" % (kb, ncu, u, rate(ncu, 1024, u)), flush=True)
    if 2 * ncu <= 512:
        print("%4d KB  %4d x  512 x %2d  %8.1f" % (kb, 2 * ncu, u, rate(2 * ncu, 512, u)), flush=True)
# the shape of the fixed probe (bench.py's measured_peak_nt): 512 x 1024 x 8, i.e. 64 MB requested over the device at once;
# per CU that is 512 * 128 KB / CUs IF the workgroups are spread evenly and all resident (two per CU on a 256-CU part)
print("%4d KB   512 x 1024 x  8  %8.1f   (the shape of bprx_probe_stream_read_nt; KB per CU = 512 * 128 / %d CUs)"
      % (512 * 128 // ncu, rate(512, 1024, 8), ncu), flush=True)
