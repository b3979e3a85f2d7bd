"""micro-benchmark of the width-64 attention core (b4r_attn_fwd_hd / b4r_attn_bwd_hd, head_dim 64) against the width-32 core at the
same hidden size (twice the heads): python tools/bench_attn64.py [B L H rate [f32|bf16x3]]"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bert4rec_amd import _lib
lib = _lib.load()
B, L, H = (int(x) for x in (sys.argv[1:4] if len(sys.argv) >= 4 else (256, 200, 128)))
rate = float(sys.argv[4]) if len(sys.argv) > 4 else 0.2
if len(sys.argv) > 5:
    _lib.check(lib.b4r_set_gemm_mode(_lib.GEMM_F32 if sys.argv[5] == "f32" else _lib.GEMM_BF16X3), "b4r_set_gemm_mode")
qkv = torch.randn(B * L, 3 * H, device="cuda") * 0.5
mask = torch.ones(B, L, dtype=torch.int64, device="cuda")
ctx = torch.empty(B * L, H, device="cuda"); lse = torch.empty(B * (H // 32) * L, device="cuda")
dctx = torch.randn(B * L, H, device="cuda"); dqkv = torch.empty(B * L, 3 * H, device="cuda")
bits = torch.empty(lib.b4r_attn_keep_words(B, L, H // 32), dtype=torch.int32, device="cuda")
state = torch.zeros(16, dtype=torch.int32, device="cuda"); state[0] = 1234
st = torch.cuda.current_stream().cuda_stream
P = lambda t: t.data_ptr()
def timeit(f, reps=100):
    for _ in range(10): f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps
for hd in (64, 32):
    heads = H // hd
    fwd = lambda: _lib.check(lib.b4r_attn_fwd_hd(P(qkv), P(mask), B, L, heads, hd, P(ctx), P(lse), P(state), 1, rate, P(bits), st), "fwd")
    bwd = lambda: _lib.check(lib.b4r_attn_bwd_hd(P(qkv), P(mask), P(ctx), P(lse), P(dctx), B, L, heads, hd, hd ** -0.5, P(dqkv),
                                                 P(state), 1, rate, P(bits), st), "bwd")
    print("B %d L %d H %d head_dim %d (%d heads), rate %.2f, mode %s: forward %.1f us  backward %.1f us" %
          (B, L, H, hd, heads, rate, "bf16x3" if lib.b4r_get_gemm_mode() == _lib.GEMM_BF16X3 else "f32", timeit(fwd), timeit(bwd)))
