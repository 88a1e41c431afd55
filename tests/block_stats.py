"""Per-channel and border error of a block output, for the block tests of the three convolutional networks (test_places_gpu.py's
stem + pool point in test_convnet_glue_gpu.py, test_faces_gpu.py, test_speakers_gpu.py) and tests/test_block_stats_host.py.

A whole-tensor mean hides one wrong channel out of 512 (0.2 % of it) and a wrong border column.  Two figures do not:
  channel   the largest, over the channels, of (mean |error| of the channel) / (RMS of that channel of the reference)
  ring      (mean |error| on the outermost ring of pixels) / (mean |error| on the interior)

The yardstick is the references alone, never the device: torch-CPU fp32 against the same network with fp16 rounding wherever
the device stores fp16 (the oracle's `fp16=True` twin).  The device's figure against fp32 may be at most FACTOR x the twin's
figure against fp32 at the same test point (the attention rule's factor).  Channels whose reference RMS is under DEAD of the
tensor's RMS are left out of the channel figure (a dead channel has no scale to measure against), at most MAX_LEFT_OUT of
them."""
import numpy as np

FACTOR = 2.0
DEAD = 0.01
MAX_LEFT_OUT = 0.05


def figures(got, want):
    """got, want: NHWC float64 -> {"channel", "ring", "left_out", "worst_channel"}"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and want.ndim == 4 and min(want.shape[1:3]) >= 3, want.shape
    err = np.abs(got - want)
    rms = np.sqrt((want ** 2).mean())
    ch_rms = np.sqrt((want ** 2).mean(axis=(0, 1, 2)))
    keep = ch_rms >= DEAD * rms
    per = np.where(keep, err.mean(axis=(0, 1, 2)) / np.where(keep, ch_rms, 1.0), 0.0)
    ring = np.ones(want.shape[1:3], bool)
    ring[1:-1, 1:-1] = False
    return {"channel": float(per.max()), "worst_channel": int(per.argmax()), "left_out": float(1 - keep.mean()),
            "ring": float(err[:, ring].mean() / err[:, ~ring].mean())}


def check(name, device, twin, want):
    """device, twin, want: NHWC outputs of the device, the fp16 twin and the fp32 reference at one test point"""
    d, t = figures(device, want), figures(twin, want)
    print(f"{name}: worst channel device {d['channel']:.3e} (channel {d['worst_channel']}) twin {t['channel']:.3e}; "
          f"ring / interior device {d['ring']:.3f} twin {t['ring']:.3f}; channels left out {d['left_out']:.3f}")
    assert d["left_out"] <= MAX_LEFT_OUT, f"{name}: {d['left_out']:.1%} of the channels are dead: choose another seed"
    assert t["channel"] > 0 and t["ring"] > 0, f"{name}: the twin has no error to measure against"
    assert d["channel"] <= FACTOR * t["channel"], f"{name}: channel {d['worst_channel']} is off by {d['channel']:.3e} of its RMS, " \
                                                  f"bar {FACTOR} x twin {t['channel']:.3e}"
    assert d["ring"] <= FACTOR * t["ring"], f"{name}: the border's error is {d['ring']:.3f} x the interior's, bar {FACTOR} x twin {t['ring']:.3f}"
    return d, t
