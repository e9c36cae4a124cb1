#!/bin/bash
# timing-only ablation of k_frames phases (results are invalid when a phase is skipped)
cd "$(dirname "$0")/.."
for m in 0 1 2 4 3 6 5 7; do
  AFX_DEBUG_SKIP=$m python bench.py --full --steps 10 --warmup 2 --cpu-clips 0 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('skip=$m', 'frames_ms=%.3f'%d['roofline']['kernels_ms_per_step']['frames'])"
done
