"""Synthetic occluder-line inputs (SURVEY.md section 8(d) generator).

Region [0, W]^2 closed by four boundary walls, plus ``n`` random occluder segments whose centres
are uniform in [0.05W, 0.95W]^2, angles uniform in [0, pi) and lengths uniform in
[lmin*W, lmax*W] (so every segment lies inside the region).  The output CSV (header x1,y1,x2,y2)
is the committed fixture; nothing downstream depends on this RNG -- re-running the script is only
needed to regenerate a fixture.

    python tests/golden/gen_synthetic.py W n seed out.csv [lmin lmax]
"""
import math
import sys

import numpy as np


def make_lines(W, n, seed=1, lmin=0.02, lmax=0.10):
    rng = np.random.default_rng(seed)
    W = float(W)
    lines = [(0.0, 0.0, W, 0.0), (W, 0.0, W, W), (W, W, 0.0, W), (0.0, W, 0.0, 0.0)]
    for _ in range(n):
        cx, cy = rng.uniform(0.05 * W, 0.95 * W, size=2)
        a = rng.uniform(0.0, math.pi)
        half = 0.5 * rng.uniform(lmin * W, lmax * W)
        dx, dy = half * math.cos(a), half * math.sin(a)
        lines.append((cx - dx, cy - dy, cx + dx, cy + dy))
    return lines


def make_lines_rect(W, H, n, seed=1, lmin=0.02, lmax=0.10):
    """make_lines on a W x H region: centres uniform in [0.05W, 0.95W] x [0.05H, 0.95H], lengths uniform in
    [lmin, lmax] * min(W, H)."""
    rng = np.random.default_rng(seed)
    W, H = float(W), float(H)
    S = min(W, H)
    lines = [(0.0, 0.0, W, 0.0), (W, 0.0, W, H), (W, H, 0.0, H), (0.0, H, 0.0, 0.0)]
    for _ in range(n):
        cx = rng.uniform(0.05 * W, 0.95 * W)
        cy = rng.uniform(0.05 * H, 0.95 * H)
        a = rng.uniform(0.0, math.pi)
        half = 0.5 * rng.uniform(lmin * S, lmax * S)
        dx, dy = half * math.cos(a), half * math.sin(a)
        lines.append((cx - dx, cy - dy, cx + dx, cy + dy))
    return lines


def make_room_map(W, room, nocc, seed, centre=None):
    """A W x W region with a walled room of side `room` around `centre` (default: the middle) and `nocc` occluders
    in it: the grid is the whole region's while the filled cells (and the cost of a CPU graph) are the room's.
    The occluders keep their place in the room wherever it stands.  Returns (region, lines [n][4], seed point
    inside the room)."""
    rng = np.random.default_rng(seed)
    x0 = y0 = W / 2 - room / 2
    if centre is not None:
        x0, y0 = centre[0] - room / 2, centre[1] - room / 2
    x1, y1 = x0 + room, y0 + room
    assert 0 < x0 and x1 < W and 0 < y0 and y1 < W, "room outside the region"
    walls = [[0, 0, W, 0], [W, 0, W, W], [W, W, 0, W], [0, W, 0, 0],
             [x0, y0, x1, y0], [x1, y0, x1, y1], [x1, y1, x0, y1], [x0, y1, x0, y0]]
    c = rng.uniform(x0 + 2, x1 - 2, size=(nocc, 2))
    c[:, 1] += y0 - x0
    ang = rng.uniform(0, np.pi, size=nocc)
    ln = rng.uniform(1.0, room / 6, size=nocc)
    d = np.stack([np.cos(ang), np.sin(ang)], 1) * (ln / 2)[:, None]
    lines = np.concatenate([np.array(walls, dtype=np.float64), np.concatenate([c - d, c + d], 1)])
    region = [0.0, 0.0, float(W), float(W)]
    seed_pt = (x0 + 1.3, y0 + 1.3)
    return region, lines, seed_pt


def make_strip_map(W, H, parts, nocc, seed):
    """A W x H strip: a closed border, `parts` partitions across the short side at even steps along the long one,
    alternately from one long wall and the other and each leaving a gap of 38 % of the short side (a search
    from one end is about `parts` levels deep), and `nocc` seeded occluders shorter than a cell.  Returns
    (region, lines [4 + parts + nocc][4], fill point)."""
    rng = np.random.default_rng(seed)
    W, H = float(W), float(H)
    walls = [[0, 0, W, 0], [W, 0, W, H], [W, H, 0, H], [0, H, 0, 0]]
    long_x = W > H
    L, S = max(W, H), min(W, H)
    for i, t in enumerate(np.linspace(L / (parts + 1), L * parts / (parts + 1), parts)):
        a, b = (0.0, S * 0.62) if i % 2 else (S * 0.38, S)
        walls.append([t + 0.37, a, t + 0.37, b] if long_x else [a, t + 0.37, b, t + 0.37])
    for _ in range(nocc):
        x = rng.uniform(1, W - 1)
        y = rng.uniform(1, H - 1)
        walls.append([x, y, x + rng.uniform(-.6, .6), y + rng.uniform(-.6, .6)])
    return [0.0, 0.0, W, H], np.array(walls, dtype=np.float64), (0.5, 0.5)


# Small walled rooms on grids whose world coordinates are not exact in FP64 (name: origin, spacing, cells a
# side, seed).  depixelate(cell) = bottom_left + spacing * index rounds at every cell, so |gy| / |gx| of a
# diagonal cell is not always exactly 1 and whichbin (pointdata.h:432-520) sends some diagonal cells to the
# sector bin next to the diagonal bin.  os07: the OS-grid origin of the barnsbury drawing with a 0.7 m grid;
# neg01: a 0.1 grid around (-1000, 1000).  The seeds are ones at which the room has the same visible set as
# its twin with unit coordinates (the occluder ends are rounded to 6 decimals, so a grazing ray can differ on
# other seeds); tests/test_noisy_rooms.py checks it.
NOISY_ROOMS = {
    "os07": ((530635.696268, 183499.852969), 0.7, 24, 6),
    "neg01": ((-1000.0, 1000.0), 0.1, 30, 11),
}


def make_noisy_room(origin, spacing, n, seed):
    """A walled room of n x n filled cells.  The layout is laid on the grid PointMap::setGrid makes (cell centres
    on multiples of the spacing): with G the grid point nearest `origin`, the border rectangle is
    [-0.4, n - 0.6]^2 in cell units from G, and three occluders shorter than 1.5 cells sit on cell corners.
    Coordinates are G + spacing * u rounded to the 6 decimals of the CSV fixtures.  The same (n, seed) gives the
    same layout in cell units on every grid: origin (0, 0) and spacing 1.0 give the room with exact
    coordinates.  Returns (region = the lines' bounding box, lines [7][4], fill point in the centre cell)."""
    rng = np.random.default_rng(seed)
    lo, hi = -0.4, n - 0.6
    u = [[lo, lo, hi, lo], [hi, lo, hi, hi], [hi, hi, lo, hi], [lo, hi, lo, lo]]
    for _ in range(3):
        c = rng.integers(2, n - 3, size=2) + 0.5
        a = rng.uniform(0.0, math.pi)
        h = 0.5 * rng.uniform(0.8, 1.4)
        d = np.round([h * math.cos(a), h * math.sin(a)], 2)
        u.append([c[0] - d[0], c[1] - d[1], c[0] + d[0], c[1] + d[1]])
    u = np.array(u, dtype=np.float64)
    G = [round(round(origin[0] / spacing) * spacing, 6), round(round(origin[1] / spacing) * spacing, 6)]
    lines = np.round(np.array(G + G, dtype=np.float64) + spacing * u, 6)
    region = [float(lines[:, [0, 2]].min()), float(lines[:, [1, 3]].min()),
              float(lines[:, [0, 2]].max()), float(lines[:, [1, 3]].max())]
    mid = n // 2 + 0.2
    fill = (round(G[0] + spacing * mid, 6), round(G[1] + spacing * mid, 6))
    return region, lines, fill


def make_plaza_map(W=1400, seed=14, origin=(0.0, 0.0), spacing=1.0):
    """An open W x W plaza: border walls and 5 occluders of length <= 1.5 cells within +-30 cells of each of the
    four points (90, 90), (W - 90, 90), (90, W - 90), (W - 90, W - 90), so that sight lines run the length of
    the map past the corners' occluders.  Cell units are placed at origin + spacing * u (the default: exact
    unit coordinates).  Returns (region, lines [24][4], fill point)."""
    rng = np.random.default_rng(seed)
    W = float(W)
    u = [[0.0, 0.0, W, 0.0], [W, 0.0, W, W], [W, W, 0.0, W], [0.0, W, 0.0, 0.0]]
    for (px, py) in ((90.0, 90.0), (W - 90.0, 90.0), (90.0, W - 90.0), (W - 90.0, W - 90.0)):
        for _ in range(5):
            cx, cy = rng.uniform(-29.0, 29.0, size=2)
            a = rng.uniform(0.0, math.pi)
            h = 0.5 * rng.uniform(0.5, 1.5)
            u.append([px + cx - h * math.cos(a), py + cy - h * math.sin(a),
                      px + cx + h * math.cos(a), py + cy + h * math.sin(a)])
    u = np.array(u, dtype=np.float64)
    o = np.array([origin[0], origin[1], origin[0], origin[1]], dtype=np.float64)
    lines = o + spacing * u
    region = [origin[0], origin[1], origin[0] + spacing * W, origin[1] + spacing * W]
    fill = (origin[0] + spacing * 0.5, origin[1] + spacing * 0.5)
    return region, lines, fill


def make_pillar_hall(W, pitch, seg=0.3, seed=1):
    """A [0, W]^2 hall with its four walls and one short "pillar" at every lattice point (i, j), i and j in
    range(pitch, W - 1, pitch): a segment of length `seg` whose centre is the lattice point jittered by +-0.1 on
    each axis and whose angle is uniform in [0, pi).  A pillar stays within 0.1 + seg / 2 of its lattice point,
    inside that cell's neighbourhood, so a fill at spacing 1 from (1.5, 1.5) reaches every interior cell.  With
    pitch 3 every filled cell is BLOCKED or next to a BLOCKED cell (an expander of the metric and angular
    searches) while sight lines stay long, and the lattice makes distances tie all the time: the priority
    queues of those searches grow to several times their LDS window.  Returns (region, lines [n][4], fill
    point)."""
    assert 0.1 + seg / 2 < 0.5, "a pillar must stay inside its lattice cell"
    rng = np.random.default_rng(seed)
    W = float(W)
    lines = [[0.0, 0.0, W, 0.0], [W, 0.0, W, W], [W, W, 0.0, W], [0.0, W, 0.0, 0.0]]
    for i in range(pitch, int(W) - 1, pitch):
        for j in range(pitch, int(W) - 1, pitch):
            cx, cy = (i, j) + rng.uniform(-0.1, 0.1, size=2)
            a = rng.uniform(0.0, math.pi)
            dx, dy = 0.5 * seg * math.cos(a), 0.5 * seg * math.sin(a)
            lines.append([cx - dx, cy - dy, cx + dx, cy + dy])
    return [0.0, 0.0, W, W], np.array(lines, dtype=np.float64), (1.5, 1.5)


def make_open_room(W):
    """A [0, W]^2 room: its four walls and nothing else.  A fill at spacing 1 from (1.5, 1.5) reaches the
    (W - 1)^2 cells (1..W-1, 1..W-1), every one of which sees every other; the cells along the walls are the
    only expanders of a metric or angular search besides its selection.  Returns (region, lines [4][4], fill
    point)."""
    W = float(W)
    lines = [[0.0, 0.0, W, 0.0], [W, 0.0, W, W], [W, W, 0.0, W], [0.0, W, 0.0, 0.0]]
    return [0.0, 0.0, W, W], np.array(lines, dtype=np.float64), (1.5, 1.5)


def write_csv(path, lines):
    with open(path, "w") as f:
        f.write("x1,y1,x2,y2\n")
        for l in lines:
            f.write("%.6f,%.6f,%.6f,%.6f\n" % tuple(l))


if __name__ == "__main__":
    if sys.argv[1] == "room":   # python tests/golden/gen_synthetic.py room os07 out.csv
        region, lines, fill = make_noisy_room(*NOISY_ROOMS[sys.argv[2]])
        write_csv(sys.argv[3], lines)
        print("fill %.6f,%.6f" % fill)
        sys.exit(0)
    W, n, seed, out =int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    lmin, lmax = (float(sys.argv[5]), float(sys.argv[6])) if len(sys.argv) > 6 else (0.02, 0.10)
    write_csv(out, make_lines(W, n, seed, lmin, lmax))
