"""How long does the host take to enqueue one step (25 frames) vs how long the GPU takes to run it?
   python tools/host_submit.py [--ops | --batch | --fused-call] [--dynamic]
   default: the fused per-frame operators (bench.py --per-frame); --ops: the operator chain; --batch: the frame batch;
   --fused-call: one call of the C ABI per frame and direction (bench.py --per-frame-fused)"""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from splatter_a_video_amd.synth import make_scene

mode = next((m for flag, m in (("--ops", "ops"), ("--batch", "batch"), ("--fused-call", "frame_fused")) if flag in sys.argv), "frame")
dev = torch.device("cuda", 0)
sc = make_scene(300000, 854, 480, F=50, C=0, seed=1234)
R = bench.FrameRenderer(sc, dev, list(range(25)), 0, mode=mode, dynamic="--dynamic" in sys.argv)
for _ in range(2):
    R.step()
R.finish(); torch.cuda.synchronize()
sub, tot = [], []
for _ in range(5):
    t0 = time.perf_counter()
    R.step()
    t1 = time.perf_counter()
    R.finish(); torch.cuda.synchronize()
    t2 = time.perf_counter()
    sub.append((t1 - t0) / 25 * 1e3); tot.append((t2 - t0) / 25 * 1e3)
print("host enqueue ms/frame", [round(x, 3) for x in sub], "total ms/frame", [round(x, 3) for x in tot])
