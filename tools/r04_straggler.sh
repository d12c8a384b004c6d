#!/bin/bash
# is the geometry tax co-residency?  busy neighbour with / without the CU's whole LDS
# (the second half, geometry kernels claiming the LDS through an environment mask, is closed: the mask is the build-time constant GSPN_GEOM_CLAIM_LDS_DEFAULT)
ms() { python -c "import json,sys; r=json.loads(sys.stdin.read()); print(round(r['ms_per_step'],3), 'fps_ms', round(r['roofline']['avg_launch_ms'],3))"; }
lay() { env "$@" GSPN_BENCH_LAYERS_ONLY=1 python bench.py --no-cpu-baseline --no-extra --steps 100 2>/dev/null | tail -1 | ms; }
full() { env "$@" python bench.py --no-cpu-baseline --no-extra --steps 100 2>/dev/null | tail -1 | ms; }
echo "layers only                         $(lay A=1)"
echo "layers + 8 x loop_valu 1024 thr     $(lay GSPN_BENCH_SIDE=spin:3:8:1024:6000)"
echo "layers + 8 x loop_valu + 160KB LDS  $(lay GSPN_BENCH_SIDE=spin:12:8:1024:6000)"
echo "layers + 1 x loop_valu 1024 thr     $(lay GSPN_BENCH_SIDE=spin:3:1:1024:6000)"
echo "layers + 1 x loop_valu + 160KB LDS  $(lay GSPN_BENCH_SIDE=spin:12:1:1024:6000)"
echo "layers + fps0                       $(lay GSPN_BENCH_SIDE=fps0)"
echo "full step                           $(full A=1)"
echo "full step (repeat)                  $(full A=1)"
