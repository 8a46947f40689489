"""The bilateral filter on a resident image, by window: pb_bilateral5 (the blind driver's 5 x 5 kernel, the baseline), pb_bilateral
at ksize 5 (the same kernel) and at 3, 7, 13, 25 (csrc/bilateral.hip).  hipEvents around each call (profile_begin /
profile_end, tag 'prefilter'), warm-up calls, then ROUNDS rounds that alternate the variants; the median per variant in us, the
taps per output and the implied taps per second.  One JSON line.  python tools/bench_bilateral.py [B H W f32|f16 ROUNDS]"""
import sys, json, ctypes, numpy as np, torch
sys.path.insert(0, '.')
from polyblur_amd.engine import Engine, _DT
from oracle import polyblur_ref as ref
B, H, W = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (1, 2160, 3840)
dt = np.float16 if len(sys.argv) > 4 and sys.argv[4] == "f16" else np.float32
ROUNDS = max(int(sys.argv[5]) if len(sys.argv) > 5 else 25, 20)
SS, SC = 5.0, 0.1
g = torch.Generator(device="cuda").manual_seed(3)
x = torch.rand((B, 3, H, W), device="cuda", generator=g).to(torch.float16 if dt == np.float16 else torch.float32).contiguous()
out = torch.empty_like(x)
torch.cuda.synchronize()
eng = Engine(0)
code = _DT[np.dtype(dt)]
variants = {"pb_bilateral5": lambda: eng._check(eng.lib.pb_bilateral5(eng.ctx, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), code, B, 3, H, W))}
for k in (5, 3, 7, 13, 25):
    variants["pb_bilateral ksize=%d" % k] = lambda k=k: eng.bilateral_ptr(x.data_ptr(), out.data_ptr(), code, (B, 3, H, W), k, SS, SC)
taps = {name: 25 if name == "pb_bilateral5" else int(name.split("=")[1]) ** 2 for name in variants}


def timed(call):
    eng.profile_begin()
    call()
    ms, launches = eng.profile_end()["prefilter"]
    assert launches == 1
    return ms * 1e3


bits = {}
for name, call in variants.items():
    for _ in range(3):
        call()
    eng.synchronize()
    bits[name] = out.clone()
us = {name: [] for name in variants}
for _ in range(ROUNDS):
    for name, call in variants.items():
        us[name].append(timed(call))
# the same small image through every variant against the oracle
small = x[:1, :, :64, :96].float().cpu().numpy().astype(dt)
err = {}
for k in (5, 3, 7, 13, 25):
    got = eng.host_call(small, lambda i, o, ex: eng.bilateral_ptr(i, o[0], code, small.shape, k, SS, SC))[0][0]
    err["ksize=%d" % k] = float(np.abs(got.astype(np.float32) - ref.bilateral_filter(small.astype(np.float32), k, SS, SC)).max())
outputs = B * 3 * H * W
print(json.dumps(dict(
    shape=[B, 3, H, W], dtype=np.dtype(dt).name, rounds=ROUNDS,
    us_median={n: round(float(np.median(t)), 1) for n, t in us.items()}, us_min={n: round(float(min(t)), 1) for n, t in us.items()},
    us_max={n: round(float(max(t)), 1) for n, t in us.items()}, taps_per_output=taps,
    tera_taps_per_s={n: round(outputs * taps[n] / (float(np.median(t)) * 1e-6) / 1e12, 3) for n, t in us.items()},
    ksize5_same_bits_as_pb_bilateral5=bool(torch.equal(bits["pb_bilateral5"], bits["pb_bilateral ksize=5"])),
    max_abs_against_oracle_64x96=err)))
