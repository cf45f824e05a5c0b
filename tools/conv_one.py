"""Launch one conv-GEMM shape repeatedly (for rocprofv3 --pmc).  Usage: python tools/conv_one.py L cin1 cin2 cout k stride ups [iters] [dtype]
or python tools/conv_one.py NAME [iters] [dtype] for a launch of the bench grid by name (NAMED below: the stride-2 downsamples, init_conv's x half
and the folded-upsampling convs; LDC_OPTIONS=lean_all=0 keeps the k = 4 / k = 7 ones on conv_fast_kernel, conv_lean=0 all of them)."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ladiffcodec_amd import lib as L  # noqa: E402

# name -> (input L, cin1, cin2, cout, k, stride, ups)
NAMED = {
    "down_256_600": (1200, 256, 0, 256, 4, 2, 0), "down_512_300": (600, 256, 0, 512, 4, 2, 0), "down_512_150": (300, 512, 0, 512, 4, 2, 0),
    "down_1024_75": (150, 512, 0, 1024, 4, 2, 0), "init_x": (1200, 128, 0, 256, 7, 1, 0),
    "up_1024_150": (75, 1024, 0, 1024, 3, 1, 1), "up_512_300": (150, 1024, 0, 512, 3, 1, 1), "up_512_600": (300, 512, 0, 512, 3, 1, 1),
    "up_256_1200": (600, 512, 0, 256, 3, 1, 1),
}
args = sys.argv[1:]
if args and args[0] in NAMED:
    args = [str(v) for v in NAMED[args[0]]] + args[1:]
Lx, c1, c2, co, k, st, ups = (int(v) for v in args[:7])
iters = int(args[7]) if len(args) > 7 else 10
dtype = args[8] if len(args) > 8 else "bf16"
Bn = int(os.environ.get("LDC_B", "32"))
lib = L.load()
cfg = L.LdcConfig()
cfg.compute_dtype = L.LDC_BF16
cfg.rep_dims, cfg.n_filters, cfg.n_residual_layers, cfg.lstm = 128, 32, 1, 2
cfg.n_enc_ratios = 1
cfg.enc_ratios[0] = 8
cfg.diff_dims = 256
ctx = C.c_void_p()
L.check(lib.ldc_create(C.byref(cfg), 0, C.byref(ctx)))
ms = C.c_double()
L.check(lib.ldc_conv_microbench(ctx, L.LDC_BF16 if dtype == "bf16" else L.LDC_F32, Bn, Lx, c1, c2, co, k, st, ups, iters, C.byref(ms)))
fl = 2.0 * Bn * (2 * Lx if ups else (Lx // 2 if st == 2 else Lx)) * co * (c1 + c2) * k
print(f"{ms.value * 1e3:.1f} us  {fl / ms.value / 1e9:.1f} TFLOP/s")
lib.ldc_destroy(ctx)
