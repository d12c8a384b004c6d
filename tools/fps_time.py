"""device time of the FPS of each SA level of the bench and of the plain on-chip kernel's size classes (torch events around 20 launches,
7 such samples per shape: median (min - max) per launch).  GSPN_FPS_MODE=resident times fps_resident_kernel where the default takes the
cell kernel; GSPN_HIP_LIB=<another build of the library> times that build, so two builds are compared by alternating processes."""
import statistics, sys, torch
sys.path.insert(0, __import__('os').path.dirname(__import__('os').path.dirname(__import__('os').path.abspath(__file__))))
import bench
from gspn_amd.tf_sampling import farthest_point_sample
for n, m in ((32768, 2048), (2048, 512), (512, 128), (16384, 1024), (8192, 2048), (4096, 1024)):
    xyz_np, _ = bench.synth(8, n, 0)
    xyz = torch.from_numpy(xyz_np).cuda()
    farthest_point_sample(m, xyz); torch.cuda.synchronize()
    us = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            farthest_point_sample(m, xyz)
        e1.record(); torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 50)
    print("fps 8x%d -> %d: %.1f us (%.1f - %.1f)" % (n, m, statistics.median(us), min(us), max(us)), flush=True)
