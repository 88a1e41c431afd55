"""Where the recogniser's confidence drift comes from (CPU, no GPU): the english_g2 oracle of tests/ocr_oracle.py run
with fp16 storage emulated stage by stage (values rounded to fp16 where the device stores fp16, fp32 arithmetic
otherwise), on tests/test_ocr_gpu.py's crops and seeded weights.  Prints, per storage choice, the worst logit drift
(relative to max |logit|) and the worst relative confidence difference on the margin-stable crops, as the GPU test
measures them.

    python tools/crnn_precision.py
"""
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from eioku_amd import ocr  # noqa: E402
from eioku_amd.synth import ocr_crops  # noqa: E402

h16 = lambda t: t.half().float()


def run(sd, imgs, vgg16, seq16):
    """vgg16: VGG weights / activations stored fp16 (K4); seq16: sequences, GEMM operands and hidden states fp16."""
    out = []
    p = "FeatureExtraction.ConvNet."

    def conv(x, name, pad=1):
        w, b = (torch.from_numpy(a) for a in ocr.fold_conv(sd, name))
        y = F.conv2d(h16(x) if vgg16 else x, h16(w) if vgg16 else w, b, padding=pad)
        return y

    act = lambda t: h16(F.relu(t)) if vgg16 else F.relu(t)
    for a in imgs:
        x = torch.from_numpy(a)[None, None]
        h = F.max_pool2d(act(conv(x, p + "0")), 2, 2)
        h = F.max_pool2d(act(conv(h, p + "3")), 2, 2)
        h = act(conv(act(conv(h, p + "6")), p + "8"))
        h = F.max_pool2d(h, (2, 1), (2, 1))
        h = act(conv(act(conv(h, p + "11")), p + "14"))
        h = act(conv(F.max_pool2d(h, (2, 1), (2, 1)), p + "18", 0))
        v = F.adaptive_avg_pool2d(h.permute(0, 3, 1, 2), (None, 1)).squeeze(3)
        q16 = h16 if seq16 else (lambda t: t)
        v = q16(v)
        for l in range(2):
            q = f"SequenceModeling.{l}."
            rnn = torch.nn.LSTM(256, 256, bidirectional=True, batch_first=True)
            st = {k[len(q + "rnn."):]: torch.from_numpy(np.asarray(sd[k], np.float32)) for k in sd if k.startswith(q + "rnn.")}
            rnn.load_state_dict({k: (q16(t) if "weight_ih" in k else t) for k, t in st.items()})
            r, _ = rnn(v)
            v = q16(F.linear(q16(r), q16(torch.from_numpy(sd[q + "linear.weight"])), torch.from_numpy(sd[q + "linear.bias"])))
        lg = F.linear(v, q16(torch.from_numpy(sd["Prediction.weight"])), torch.from_numpy(sd["Prediction.bias"]))[0]
        pr = ocr.ignore_renormalise(F.softmax(lg, -1).numpy(), [])
        out.append((pr.argmax(-1), pr.max(-1), lg.numpy()))
    return out


def main():
    sd = ocr._np_state(ocr.random_crnn_state(6))
    imgs = ocr_crops(1, [64, 192, 128, 64, 320, 192, 64, 128, 256])
    with torch.no_grad():
        ref = run(sd, imgs, False, False)
        for label, cfg in (("fp16 VGG, fp16 sequence path", (True, True)), ("fp16 VGG, fp32 sequence path", (True, False)),
                           ("fp32 VGG, fp16 sequence path", (False, True))):
            got = run(sd, imgs, *cfg)
            wl = wc = 0.0
            for (gi, gp, gl), (ri, rp, rl) in zip(got, ref):
                wl = max(wl, float(np.abs(gl - rl).max() / np.abs(rl).max()))
                srt = np.sort(rl, -1)
                if (srt[:, -1] - srt[:, -2]).min() > 4 * np.abs(gl - rl).max():
                    cg, cr = ocr.confidence(gi, gp), ocr.confidence(ri, rp)
                    wc = max(wc, abs(cg - cr) / max(cr, 1e-30))
            print(f"{label:32s} logits {wl:.2e}  confidence {wc:.2e}")


if __name__ == "__main__":
    main()
