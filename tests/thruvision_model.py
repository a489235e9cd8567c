"""numpy restatement of VGA through vision (VGAThroughVision::run, salalib/vgamodules/vgathroughvision.cpp:27-104,
over PixelBase::quickPixelateLine, salalib/spacepix.cpp:218-270).  Test infrastructure only.

For every source s and every cell x that Node::first()..next() yields for s's node, the line p = x -> q = s is
walked: dx = q.x - p.x, dy = q.y - p.y as doubles; |dx| == |dy| emits one pixel and counts nothing; otherwise
t = max(|dx|, |dy|), dx /= t, dy /= t, pp = p + 0.5, and for i = 0..t a pixel is emitted and THEN pp += (dx, dy),
accumulated in FP64 step by step.  In the major-x case a pp.y within 1e-9 above an integer (fabs(floor(ppy) - ppy)
< 1e-9) emits the two pixels floor(ppy + 0.5) and floor(ppy - 0.5); the major-y case is symmetric.  Everything
emitted at iterations 1..t-1 counts once; the first and last list entries (p and q) do not.

numpy's float64 add, divide and floor are the IEEE operations the reference's doubles use, so the walk is
vectorised over lines and loops over the step index."""
import numpy as np


def walk(p, q):
    """The reference's pixel list for one line, as a list (one entry per iteration) of lists of (x, y)."""
    dx, dy = np.float64(q[0] - p[0]), np.float64(q[1] - p[1])
    if abs(dx) == abs(dy):
        return [[(int(p[0]), int(p[1]))]]
    major_x = abs(dx) > abs(dy)
    t = abs(dx) if major_x else abs(dy)
    dx, dy = dx / t, dy / t
    ppx, ppy = np.float64(p[0]) + 0.5, np.float64(p[1]) + 0.5
    out = []
    for _ in range(int(t) + 1):
        fx, fy = np.floor(ppx), np.floor(ppy)
        if major_x and abs(fy - ppy) < 1e-9:
            out.append([(int(fx), int(np.floor(ppy + 0.5))), (int(fx), int(np.floor(ppy - 0.5)))])
        elif not major_x and abs(fx - ppx) < 1e-9:
            out.append([(int(np.floor(ppx + 0.5)), int(fy)), (int(np.floor(ppx - 0.5)), int(fy))])
        else:
            out.append([(int(fx), int(fy))])
        ppx, ppy = ppx + dx, ppy + dy
    return out


def line_counts(cols, rows, src, vis):
    """src, vis: int arrays [L][2] of (x, y); every line is walked from vis (p) to src (q).  Returns the
    counts as int64 [cols * rows], x-major."""
    src, vis = np.asarray(src).reshape(-1, 2), np.asarray(vis).reshape(-1, 2)
    px, py = vis[:, 0].astype(np.float64), vis[:, 1].astype(np.float64)
    dx, dy = src[:, 0] - px, src[:, 1] - py
    adx, ady = np.abs(dx), np.abs(dy)
    keep = adx != ady
    px, py, dx, dy, adx, ady = (a[keep] for a in (px, py, dx, dy, adx, ady))
    mx = adx > ady
    t = np.where(mx, adx, ady)
    dx, dy = dx / t, dy / t
    ppx, ppy = px + 0.5, py + 0.5
    cnt = np.zeros(cols * rows, np.int64)

    def add(x, y, m):
        if m.any():
            cnt[:] += np.bincount(x[m].astype(np.int64) * rows + y[m].astype(np.int64), minlength=cols * rows)

    for i in range(1, int(t.max()) if len(t) else 0):
        ppx, ppy = ppx + dx, ppy + dy
        live = i < t   # iterations 1 .. t - 1
        fx, fy = np.floor(ppx), np.floor(ppy)
        h1 = live & mx & (np.abs(fy - ppy) < 1e-9)
        h2 = live & ~mx & (np.abs(fx - ppx) < 1e-9)
        add(fx, fy, live & ~h1 & ~h2)
        add(fx, np.floor(ppy + 0.5), h1)
        add(fx, np.floor(ppy - 0.5), h1)
        add(np.floor(ppx + 0.5), fy, h2)
        add(np.floor(ppx - 0.5), fy, h2)
    return cnt


def run_cells(runs):
    """The cells Node::first()..next() yields for runs [R][4] (x0, y0, x1, y1), in order, with the index of the
    run each came from: (cells [K][2], run_index [K]).  A run yields its start cell and steps along its direction
    (y0 == y1: x, x0 == x1: y, else the diagonal) to its end; never fewer than one cell (Bin::next,
    ngraph.cpp:399-406)."""
    r = np.asarray(runs, dtype=np.int64).reshape(-1, 4)
    vert = (r[:, 0] == r[:, 2]) & (r[:, 1] != r[:, 3])
    n = np.maximum(np.where(vert, r[:, 3] - r[:, 1], r[:, 2] - r[:, 0]) + 1, 1)
    idx = np.repeat(np.arange(len(r)), n)
    k = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    sx = np.where(vert, 0, 1)[idx]
    sy = np.where(r[:, 1] == r[:, 3], 0, np.where(r[:, 3] > r[:, 1], 1, -1))[idx]
    return np.stack([r[idx, 0] + k * sx, r[idx, 1] + k * sy], axis=1), idx


def through_vision(cols, rows, state, nruns, runs, src_begin=0, src_end=-1, batch=400000):
    """Counts per node (int64 [N], node = filled cell in x-major order) added by the sources
    [src_begin, src_end): state is Point::m_state per cell (bit 1 = FILLED), nruns [N] the runs of each node,
    runs [R][4] all runs in node order."""
    node_cell = np.flatnonzero(np.asarray(state) & 2)
    N = len(node_cell)
    if src_end < 0 or src_end > N:
        src_end = N
    nruns = np.asarray(nruns, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(nruns)])
    runs = np.asarray(runs).reshape(-1, 4)
    cnt = np.zeros(cols * rows, np.int64)
    s = src_begin
    while s < src_end:
        e = s + 1
        while e < src_end and start[e + 1] - start[s] < batch // 8:
            e += 1
        cells, ridx = run_cells(runs[start[s]:start[e]])
        node = np.searchsorted(start, ridx + start[s], side="right") - 1
        src = np.stack([node_cell[node] // rows, node_cell[node] % rows], axis=1)
        inside = (cells[:, 0] >= 0) & (cells[:, 0] < cols) & (cells[:, 1] >= 0) & (cells[:, 1] < rows)
        cnt += line_counts(cols, rows, src[inside], cells[inside])
        s = e
    return cnt[node_cell]
