"""Time one margin head at batch 256, 28 000 classes, 512 features: `iters` forward calls (mode fwd) or forward + backward
calls (mode fwdbwd) after 3 warm-up calls, event-timed; run it under `rocprofv3 --kernel-trace --stats -- ...` for the
kernel times (profiles/margin_heads_b256_n28000.txt).

    python tools/head_time.py {ArcFace|CosFace|SphereFace|Am_softmax} {fwd|fwdbwd} ITERS
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stylegan-for-facerec_amd"), ROOT]
import torch  # noqa: E402
from frhip import synth, functional as FRF  # noqa: E402
from head import metrics as H  # noqa: E402

name, mode, iters = sys.argv[1], sys.argv[2], int(sys.argv[3])
B, D, N = 256, 512, 28000
FRF.CHECK_LABELS = False
head = getattr(H, name)(D, N, None).cuda()
x = synth.normal(5, "t.x", (B, D)).cuda().requires_grad_(mode == "fwdbwd")
label = synth.labels(5, "t.y", B, N).cuda()
g = synth.normal(5, "t.g", (B, N)).cuda()
p = list(head.parameters())[0]


def step():
    y = head(x, label)
    if mode == "fwdbwd":
        x.grad = None
        p.grad = None
        y.backward(g)


for _ in range(3):
    step()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(iters):
    step()
e1.record()
torch.cuda.synchronize()
print("HEADTIME %s %s %.1f us/call (events, %d calls)" % (name, mode, e0.elapsed_time(e1) * 1e3 / iters, iters))
