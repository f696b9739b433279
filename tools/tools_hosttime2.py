import sys, time, os
sys.path.insert(0, '.')
import torch, numpy as np, ctypes as C
import visual_odometry_ros_amd as V
from visual_odometry_ros_amd import api
orig = api.StereoFramePipeline.enqueue_device
cnt = [0]; hist = []
def g(self, *a, **k):
    t0 = time.perf_counter()
    dT = api._f32(a[4]).reshape(16)
    t1 = time.perf_counter()
    r = orig(self, *a, **k)
    t2 = time.perf_counter()
    cnt[0] += 1
    hist.append(1e6*(t2-t1))
    if cnt[0] % 50 == 0:
        print(f"py: calls {cnt[0]-49}..{cnt[0]}: mean {sum(hist[-50:])/50:.1f} us, max {max(hist[-50:]):.1f}", file=sys.stderr)
    return r
api.StereoFramePipeline.enqueue_device = g
import runpy, gc
if os.environ.get('NOGC'): gc.disable()
sys.argv = ["bench.py", "--full", "--no-cpu-baseline", "--strict-border", "0", "--steps", "400", "--warmup", "5"]
runpy.run_path("bench.py", run_name="__main__")
