"""Time the head's last steps at the headline shape: y6 [1,12,32,64,208] -> upsample x2 -> last_3_3d (12 -> 1) -> mat [1,1,64,128,416].
   (a) the fused kernel ragmi_upconv3d_c1_fwd; (b) standalone upsample + convolution (conv3d_c1 / generic small-Cout kernel);
   (c) the tap form from level 12 (ragmi_trilinear3d_act_k1_fwd -> ragmi_uptaps3d_fwd) against the same two launches of the channel form;
   (d) the tap form with the x blend in the resample launch (ragmi_trilinear3d_act_k1_xblend_fwd -> ragmi_uptaps3d_xblended_fwd).
    python tools/bench_head.py"""
import os
import sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rag_amd as ra  # noqa: E402

dev = "cuda:0"
y6 = torch.randn((1, 12, 32, 64, 208), device=dev)
shape = (1, 12, 64, 128, 416)
ups = [torch.empty(shape, device=dev) for _ in range(2)]       # 2 x 164 MB in rotation: past the 256 MiB memory-side cache
w = torch.randn((1, 12, 3, 3, 3), device=dev) * 0.05
out = torch.empty((1, 1) + shape[2:], device=dev)


def timed(fn, n=40):
    for i in range(4):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def two(i):
    ra.ops.trilinear3d_act(y6, shape[2:], True, False, ups[i % 2], 0)
    ra.ops.conv3d_k3_small(ups[i % 2], w, None, None, False, out)


t_conv = timed(lambda i: ra.ops.conv3d_k3_small(ups[i % 2], w, None, None, False, out))
t_two = timed(two)
t_fused = timed(lambda i: ra.ops.upconv3d_c1(y6, w, None, None, False, out))
print(f"last_3_3d alone {t_conv:.1f} us; upsample + last_3_3d {t_two:.1f} us; fused upconv3d_c1 {t_fused:.1f} us "
      f"({2 * 27 * 12 * out.numel() / t_fused / 1e6:.1f} TFLOP/s)")

# (c) the tap form from one level lower, as MatchingNet._head runs it: low [1,12,16,32,104] -> resample + ReLU (+ the 12 -> 27 mix) ->
# head kernel, against the same two launches of the channel form (trilinear3d_act -> upconv3d_c1)
low = torch.randn((1, 12, 16, 32, 104), device=dev)
y6b = torch.empty_like(y6)
p6 = torch.empty((1, 27) + tuple(y6.shape[2:]), device=dev)


def channel_pair(i):
    ra.ops.trilinear3d_act(low, y6.shape[2:], True, True, y6b, 0)
    ra.ops.upconv3d_c1(y6b, w, None, None, False, out)


def tap_pair(i):
    ra.ops.trilinear3d_act_k1(low, y6.shape[2:], True, True, w, p6, 0, transposed=True)
    ra.ops.uptaps3d(p6, None, None, False, out)


t_ch, t_tap = timed(channel_pair), timed(tap_pair)
t_k1 = timed(lambda i: ra.ops.trilinear3d_act_k1(low, y6.shape[2:], True, True, w, p6, 0, transposed=True))
t_ut = timed(lambda i: ra.ops.uptaps3d(p6, None, None, False, out))
print(f"head from level 12: trilinear3d_act + upconv3d_c1 {t_ch:.1f} us; trilinear3d_act_k1 + uptaps3d {t_tap:.1f} us "
      f"(trilinear3d_act_k1 alone {t_k1:.1f} us, uptaps3d alone {t_ut:.1f} us)")

# (d) the x blend of the taps taken in the resample launch: Q [1,9,32,64,416] between the two
q6 = torch.empty((1, 9) + tuple(y6.shape[2:4]) + (2 * y6.shape[4],), device=dev)


def xblend_pair(i):
    ra.ops.trilinear3d_act_k1(low, y6.shape[2:], True, True, w, q6, 0, transposed=True, xblend=True)
    ra.ops.uptaps3d(q6, None, None, False, out, xblended=True)


tap_pair(0)
ref = out.clone()
xblend_pair(0)
t_xb = timed(xblend_pair)
t_xk1 = timed(lambda i: ra.ops.trilinear3d_act_k1(low, y6.shape[2:], True, True, w, q6, 0, transposed=True, xblend=True))
t_xut = timed(lambda i: ra.ops.uptaps3d(q6, None, None, False, out, xblended=True))
print(f"head from level 12, x blend in the resample launch: pair {t_xb:.1f} us (trilinear3d_act_k1 xblend alone {t_xk1:.1f} us, "
      f"uptaps3d xblended alone {t_xut:.1f} us); output bits equal to the tap pair's: {torch.equal(out, ref)}")
