"""Per-workgroup start / end ticks of k_fft and k_fm in the side-by-side step (a -DJSDR_X_WGCLK build named by JSDR_LIB).
   python tools/wgclk_probe.py <steps>   -> the CSVs named by JSDR_X_WGCLK_OUT / JSDR_X_WGCLK_OUT_FM (profiles/r09_ticket_handout.md)"""
import gc
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import java_sdr_amd as J  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
S, L = 8192, 1 << 20
d_iq, pay, nfr = bench.make_inputs(J, S, L, 0)
nframes = S * L // 2048
fft = J.Fft(2048, 96000)
d_psd = J.DeviceBuffer(nframes * 2050 * 4)
dem = J.Bpsk(rate=96000, blen=4 * 2048, tuning=12000, do_fft=0, nstreams=S, max_batch_samples=L, variant="exact")
shares = dem.pair_shares()
print("shares", shares, flush=True)
fft.set_cu_share(shares[0])
dem.set_cu_share(shares[1])
ms, ps = J.Stream(), J.Stream()


def sync():
    ps.sync()
    ms.sync()
    dem.sync()
    J.binding.stream_sync(None)


for i in range(3):
    fft.batch_i16(d_iq, nframes, d_psd, stream=ps.ptr)
    dem.batch_i16(d_iq, 2 * L, L, stream=ms.ptr)
sync()
t0 = time.perf_counter()
for i in range(steps):
    fft.batch_i16(d_iq, nframes, d_psd, stream=ps.ptr)
    dem.batch_i16(d_iq, 2 * L, L, stream=ms.ptr)
sync()
print("ms per step", (time.perf_counter() - t0) / steps * 1e3, "fft", fft.last_launch(), "fm", dem.last_launch(), dem.front_kernel_name(), flush=True)
del fft
del dem
gc.collect()
print("done", flush=True)
