"""numpy restatement of mpnn_conf_gate (include/mpnn_hip.h, csrc/conf_gate.hip): the confidence-threshold exit decision
of one switch, sample by sample, in plain loops.

    for every sample s < min(cnt, n) (s < n without a count), img = idx[s] (s without a list):
        d = exit_sink                                       if conf[img] >= tau   (float32; a NaN on either side: no)
        d = arg-max of r[img][i] over i != exit_sink        otherwise             (first index on ties)
        r[img][i] = 1 if i == d else 0                      for i < n_sinks
        img joins the child set of sink d

Nothing here is shared with the kernel or with the engine: the comparison is numpy's float32 `>=`, the arg-max a loop
with `>` that starts from the first candidate (so a NaN first candidate stays, as in tf.argmax's first-index rule applied
by exit_ev_k)."""
import numpy as np


def gate(conf, tau, r, n_sinks, exit_sink, idx=None, cnt=None, n=None):
    """conf: [images] float32; tau: one float32; r: [images, r_stride] float32 (not modified); idx: the sample list or
    None; cnt: the count on the device or None; n: the capacity (default: len(idx) or len(conf)).

    Returns dict(imgs=the images handled, in list order; d={img: decision}; rows=r after the launch (a copy; rows of
    other images and the columns from n_sinks on keep their bits); children=[sorted int array per sink])."""
    conf = np.asarray(conf, np.float32)
    tau = np.float32(tau)
    rows = np.array(r, np.float32, copy=True)
    if n is None:
        n = len(idx) if idx is not None else len(conf)
    m = n if cnt is None else min(int(cnt), n)
    imgs = [int(idx[s]) if idx is not None else s for s in range(max(m, 0))]
    d = {}
    children = [[] for _ in range(n_sinks)]
    for img in imgs:
        with np.errstate(invalid='ignore'):
            leave = bool(conf[img] >= tau)
        if leave:
            k = exit_sink
        else:
            k, best = None, None
            for i in range(n_sinks):
                if i == exit_sink:
                    continue
                v = r[img][i]
                if k is None or v > best:
                    k, best = i, v
        d[img] = k
        for i in range(n_sinks):
            rows[img, i] = 1.0 if i == k else 0.0
        children[k].append(img)
    return dict(imgs=imgs, d=d, rows=rows, children=[np.sort(np.array(c, np.int64)) for c in children])
