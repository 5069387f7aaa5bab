"""Time one head at batch 256, 28 000 classes, 512 features: `iters` forward calls (mode fwd) or forward + backward
calls (mode fwdbwd) after 3 warm-up calls, event-timed; run it under `rocprofv3 --kernel-trace --stats -- ...` for the
kernel times (profiles/margin_heads_b256_n28000.txt).

    python tools/head_time.py {ArcFace|CosFace|SphereFace|Am_softmax|CurricularFace|MagFace|AdaCos|NPCFace|MV_Softmax|MV_Softmax-arc
                               |CircleLoss|AM_Softmax|ArcNegFace|Softmax} {fwd|fwdbwd} ITERS

Several heads, comma separated, are timed in ONE process in alternating rounds (ROUNDS rounds of ITERS calls per head, the
median round of each head reported, and the ratio to the first head named), so clocks and allocator state are shared
(profiles/curricular_head_b256_n28000.txt, profiles/magface_head_b256_n28000.txt,
profiles/adacos_head_b256_n28000.txt, profiles/npcface_head_b256_n28000.txt, profiles/mv_softmax_head_b256_n28000.txt,
profiles/circle_heads_b256_n28000.txt, profiles/arcnegface_head_b256_n28000.txt, profiles/softmax_head_b256_n28000.txt;
MV_Softmax is the additive-margin form, MV_Softmax-arc the ArcFace-style one; Softmax is the plain linear head with a bias):

    python tools/head_time.py Am_softmax,ArcFace,CurricularFace fwdbwd ITERS [ROUNDS]

MagFace returns (logits, loss_g); its backward call takes ``g`` for the logits and ones / B for loss_g (train.py's
``loss_g.mean()``), so both of its radial terms are in the timed path.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stylegan-for-facerec_amd"), ROOT]
import torch  # noqa: E402
from frhip import synth, functional as FRF  # noqa: E402
from head import metrics as H  # noqa: E402

names, mode, iters = sys.argv[1].split(","), sys.argv[2], int(sys.argv[3])
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 5
B, D, N = 256, 512, 28000
FRF.CHECK_LABELS = False
x = synth.normal(5, "t.x", (B, D)).cuda().requires_grad_(mode == "fwdbwd")
label = synth.labels(5, "t.y", B, N).cuda()
g = synth.normal(5, "t.g", (B, N)).cuda()
gg = torch.full((B, 1), 1.0 / B).cuda()


def make(name):
    zoo = name in ("CurricularFace", "MagFace", "AdaCos", "NPCFace", "CircleLoss", "AM_Softmax", "ArcNegFace")  # FaceX-Zoo heads: no device_id
    if name in ("MV_Softmax", "MV_Softmax-arc"):  # is_am is a required argument: the AM form, or the ArcFace-style one
        head = H.MV_Softmax(D, N, name == "MV_Softmax").cuda()
    else:
        cls = getattr(H, name)
        head = (cls(D, N) if zoo else cls(D, N, None)).cuda()
    params = list(head.parameters())  # one parameter; the Softmax head's bias is a second

    def step():
        y = head(x, label)
        if mode == "fwdbwd":
            x.grad = None
            for p in params:
                p.grad = None
            if isinstance(y, tuple):
                torch.autograd.backward(y, [g, gg])
            else:
                y.backward(g)

    return step


def timed(step, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


steps = {name: make(name) for name in names}
for step in steps.values():
    for _ in range(3):
        step()
torch.cuda.synchronize()
if len(names) == 1:
    print("HEADTIME %s %s %.1f us/call (events, %d calls)" % (names[0], mode, timed(steps[names[0]], iters), iters))
else:
    per = {name: [] for name in names}
    for _ in range(rounds):
        for name in names:
            per[name].append(timed(steps[name], iters))
    med = {name: sorted(v)[len(v) // 2] for name, v in per.items()}
    for name in names:
        print("HEADTIME %-14s %s median %.1f us/call, rounds %s, %.3f x %s (events, %d rounds of %d calls, alternating)"
              % (name, mode, med[name], " ".join("%.1f" % t for t in per[name]), med[name] / med[names[0]], names[0],
                 rounds, iters))
