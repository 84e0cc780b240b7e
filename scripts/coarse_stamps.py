"""Diagnostic: per-section cycle totals of the coarse FFT kernel (wave 0 of
every workgroup that ran a hop) from the AERO_X_STAMPS build: the sections of
a hop, lane 0's hop control, and what is left of the workgroup's time in the
kernel (the turnover between channels: launch, batch scans, waits for the
other waves at a channel's first barrier).
Usage: AERO_ENGINE_SO=aero-cli_amd/libaero_engine_stamps.so python scripts/coarse_stamps.py [channels]"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'aero-cli_amd'), os.path.join(ROOT, 'tests'), ROOT]
import bench  # noqa: E402
import shard  # noqa: E402

C = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
M = bench.MODES['oqpsk10500']
P = min(64, C)
steps = 56
offs = shard.channel_offsets(C, P, 0)
pool_host = bench.make_pool(M, P, steps * 4096 + int(offs.max()) + 1, 0xAE20)
import torch  # noqa: E402
import aero_engine as ae  # noqa: E402
pool = torch.from_numpy(pool_host).to('cuda')
eng = ae.Engine(max_channels=C)
for _ in range(C):
    eng.open_channel(10500, 48000)
lib = ae.load_library()
fn = lib.aero_x_coarse_stamps
fn.argtypes = [ctypes.c_void_p]
out = (ctypes.c_ulonglong * 12)()
vfn = lib.aero_x_viterbi_stamps
vfn.argtypes = [ctypes.c_void_p]
vout = (ctypes.c_ulonglong * 4)()
# With the overlapped head (the default; AERO_COARSE_OVERLAP=0 for the plain one) a channel that
# follows another in its batch has no head of its own: slots 0 and 1 then count the plain heads
# only (a batch's first due channel), slot 2 the serial rest (the successor's mix), and the
# successor's image loads, the barrier inside |X| and the issue of its table gathers run inside
# slot 6, the twiddle write at the head of slot 7, under which the gathers land.  What the other waves
# wait for lane 0's hop control shows in wave 0's figures only as the kernel time per hop.
names = ['batch scan + state (plain heads)', 'ring to LDS (plain heads)', 'gathers + mix / serial mix', 'FFT 1',
         'boxcar+iFFT+square', 'FFT 3', 'hypot + next image, gathers', 'twiddles + log10',
         'fold', 'hop control (lane 0)']
order = list(range(10))
for s in range(steps):
    views = [pool[:, int(o) + s * 4096:int(o) + (s + 1) * 4096] for o in offs]
    x = torch.stack(views).permute(2, 0, 1).reshape(4096, C).contiguous()
    torch.cuda.synchronize()
    eng.push_batch_device(x.data_ptr(), 4096, C, C)
    eng.run()
    eng.sync()
    if s == 47:
        fn(out)  # reset after the lock-in pre-roll
        vfn(vout)
fn(out)
vfn(vout)
tot = sum(out[:10])
n = out[11]
print('channels %d, hops %d, s_memtime cycles per hop (wave 0) %.0f' % (C, n, tot / max(n, 1)))
for k in order:
    print('  %-34s %9.0f  %5.1f %%' % (names[k], out[k] / max(n, 1), 100.0 * out[k] / max(tot, 1)))
if out[10]:  # the persistent kernel: wave 0's whole time in the kernel
    print('  %-34s %9.0f  (kernel time per hop %.0f)' % ('turnover', (out[10] - tot) / max(n, 1), out[10] / max(n, 1)))
eng.close()
vn = vout[3]
print('viterbi jobs %d, s_memtime cycles per job %.0f' % (vn, sum(vout[:3]) / max(vn, 1)))
for k, nm in enumerate(['load + deinterleave', 'decode', 'delay line, descramble, CRC, record']):
    print('  %-38s %9.0f' % (nm, vout[k] / max(vn, 1)))
