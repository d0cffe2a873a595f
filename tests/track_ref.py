"""The track rule of lanpaint_amd/detail.py restated plainly: one loop per frame and per step, no helper shared with the package.
`plan_track_ref` returns (H, W, h, w, oh, ow, origins) as plain integers and tuples."""


def _axis_ref(spans, N, c, padding, M, k):
    F = len(spans)
    # centre
    s = []
    for f in range(F):
        if spans[f] is None:
            s.append(None)
        else:
            s.append(spans[f][0] + spans[f][1] + 1)
    # fill
    filled = list(s)
    for f in range(F):
        if s[f] is not None:
            continue
        p = f - 1
        while p >= 0 and s[p] is None:
            p -= 1
        q = f + 1
        while q < F and s[q] is None:
            q += 1
        if p >= 0 and q < F:
            filled[f] = s[p] + ((s[q] - s[p]) * (f - p)) // (q - p)
        elif p >= 0:
            filled[f] = s[p]
        else:
            filled[f] = s[q]
    # size
    side = 0
    for f in range(F):
        if spans[f] is not None and spans[f][1] - spans[f][0] + 1 > side:
            side = spans[f][1] - spans[f][0] + 1
    grow_num = (c - 1000) * side
    g = padding + (grow_num + 1999) // 2000
    n = side + 2 * g
    if n > N:
        n = N
    need = ((n + M - 1) // M) * M
    if need <= N:
        n = need
    # smooth, contain, clamp
    r = k // 2
    los = []
    for f in range(F):
        S = 0
        for j in range(-r, r + 1):
            i = f + j
            if i < 0:
                i = 0
            if i > F - 1:
                i = F - 1
            S += filled[i]
        lo = (S - k * n) // (2 * k)
        if spans[f] is not None:
            if lo > spans[f][0]:
                lo = spans[f][0]
            if lo < spans[f][1] + 1 - n:
                lo = spans[f][1] + 1 - n
        if lo < 0:
            lo = 0
        if lo > N - n:
            lo = N - n
        los.append(lo)
    return los, n


def plan_track_ref(boxes, H, W, context, padding, M, target, smooth, frames=None):
    boxes = [tuple(b) for b in boxes]
    if frames is not None and len(boxes) == 1:
        boxes = boxes * frames
    c = int(round(context * 1000))
    rows, cols = [], []
    for r0, r1, c0, c1 in boxes:
        empty = r1 < r0 or c1 < c0
        rows.append(None if empty else (r0, r1))
        cols.append(None if empty else (c0, c1))
    ys, h = _axis_ref(rows, H, c, padding, M, smooth)
    xs, w = _axis_ref(cols, W, c, padding, M, smooth)
    if target <= 0:
        oh, ow = h, w
    else:
        L = h if h > w else w
        oh = (2 * h * target + L * M) // (2 * L * M)
        ow = (2 * w * target + L * M) // (2 * L * M)
        oh = (oh if oh > 1 else 1) * M
        ow = (ow if ow > 1 else 1) * M
    return H, W, h, w, oh, ow, tuple(zip(ys, xs))
