"""TEST INFRASTRUCTURE: the masks, the hand-made vote images and the oracle of the shadow-region launches
(include/hypel.h, hypel_components_*), shared by tests/test_components_emu.py and tests/test_gpu_components.py.

The oracle is the definition itself in plain integer Python: a breadth-first flood fill over the 8-neighbourhood started
at every unvisited mask pixel in row-major order (so a component's root is the pixel it was started from and its id the
number of components started before it), then one loop over the component pixels and their neighbours for the votes."""
import functools

import numpy as np

N_CLASSES, SHADOW, BUILDING = 11, 6, 7
EXCLUDE = (SHADOW, BUILDING)
NEIGHBOURS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


# ----------------------------------------------------------------------------------------------------- oracle
def flood_fill(mask):
    """-> (root int32 [h, w], comp int32 [h, w], n, size int32 [n]) of the 8-connected components of mask != 0"""
    mask = np.asarray(mask)
    h, w = mask.shape
    pw = w + 2  # one pixel of padding all round: no bounds checks in the loop
    padded = np.zeros((h + 2, pw), np.uint8)
    padded[1:-1, 1:-1] = mask != 0
    todo = bytearray(padded.tobytes())
    root_of, comp_of = [-1] * len(todo), [-1] * len(todo)
    steps = [dy * pw + dx for dy, dx in NEIGHBOURS]
    sizes = []
    for start in range(len(todo)):
        if not todo[start]:
            continue
        first = (start // pw - 1) * w + start % pw - 1
        ident = len(sizes)
        queue, head = [start], 0
        todo[start] = 0
        while head < len(queue):
            p = queue[head]
            head += 1
            root_of[p], comp_of[p] = first, ident
            for s in steps:
                if todo[p + s]:
                    todo[p + s] = 0
                    queue.append(p + s)
        sizes.append(len(queue))
    root = np.array(root_of, np.int32).reshape(h + 2, pw)[1:-1, 1:-1]
    comp = np.array(comp_of, np.int32).reshape(h + 2, pw)[1:-1, 1:-1]
    return np.ascontiguousarray(root), np.ascontiguousarray(comp), len(sizes), np.array(sizes, np.int32).reshape(-1)


def count_votes(targets, comp, n, n_classes=N_CLASSES, exclude=EXCLUDE):
    """-> (votes int32 [n, n_classes], winner uint8 [n])"""
    h, w = comp.shape
    t, c = targets.tolist(), comp.tolist()
    votes = [[0] * n_classes for _ in range(n)]
    for y in range(h):
        for x in range(w):
            if c[y][x] < 0:
                continue
            for dy, dx in NEIGHBOURS:
                qy, qx = y + dy, x + dx
                if 0 <= qy < h and 0 <= qx < w and c[qy][qx] < 0:
                    cls = t[qy][qx]
                    if cls < n_classes and cls not in exclude:
                        votes[c[y][x]][cls] += 1
    winner = []
    for row in votes:
        best, most = 255, 0
        for cls, v in enumerate(row):
            if v > most:
                best, most = cls, v
        winner.append(best)
    return np.array(votes, np.int32).reshape(n, n_classes), np.array(winner, np.uint8).reshape(-1)


def relabel(targets, comp, winner, plus_one=False):
    out = targets.copy()
    for y, x in zip(*np.nonzero(comp >= 0)):
        if winner[comp[y, x]] != 255:
            out[y, x] = winner[comp[y, x]]
    if plus_one:
        out[out != 255] += 1
    return out


# ----------------------------------------------------------------------------------------------------- masks
def _spiral(h, w):
    """a one-pixel-wide path winding inwards, one lit pixel between its arms"""
    m = np.zeros((h, w), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    while True:
        for _ in range(2):
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= fy < h and 0 <= fx < w and m[fy, fx]):
                y, x = ny, nx
                m[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            return m


def _rings(n):
    m = np.zeros((n, n), np.uint8)
    for k in range(0, n // 2 + 1, 2):
        m[k, k:n - k] = m[n - 1 - k, k:n - k] = 1
        m[k:n - k, k] = m[k:n - k, n - 1 - k] = 1
    return m


def _combs(h, w):
    """a comb over the upper half (spine along the top, a tooth in every second column) and nested U shapes, each as
    wide as what is left of the image, below it"""
    m = np.zeros((h, w), np.uint8)
    m[0, :] = 1
    m[0:h // 2, ::2] = 1
    top = h // 2 + 2
    for k in range(0, 48, 2):
        m[top:h - k, k] = m[top:h - k, w - 1 - k] = 1
        m[h - 1 - k, k:w - k] = 1
    return m


def _corners(h, w):
    m = np.zeros((h, w), np.uint8)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 1
    return m


def _random(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8)


def _lattice(h, w):
    m = np.zeros((h, w), np.uint8)
    m[::2, ::2] = 1
    return m


def _diagonals(n, both):
    m = np.eye(n, dtype=np.uint8)
    return m | m[:, ::-1] if both else m


MASKS = {
    "empty": lambda: np.zeros((37, 70), np.uint8),
    "full": lambda: np.full((37, 130), 255, np.uint8),  # any non-zero value is inside
    "corners": lambda: _corners(33, 70),
    "row_1x97": lambda: _random(1, 97, 0.6, 1),
    "column_97x1": lambda: _random(97, 1, 0.6, 2),
    "checkerboard_33x65": lambda: (np.add.outer(np.arange(33), np.arange(65)) % 2 == 0).astype(np.uint8),
    "diagonal_130": lambda: _diagonals(130, False),
    "crossing_diagonals_130": lambda: _diagonals(130, True),
    "spiral_97x131": lambda: _spiral(97, 131),
    "rings_81": lambda: _rings(81),
    "combs_200x333": lambda: _combs(200, 333),
    "lattice_130x70": lambda: _lattice(130, 70),
    "random_0.30": lambda: _random(257, 193, 0.30, 30),
    "random_0.45": lambda: _random(257, 193, 0.45, 45),
    "random_0.60": lambda: _random(257, 193, 0.60, 60),
    "random_0.45_1202x1194": lambda: _random(1202, 1194, 0.45, 7),
}
RANDOM_WITH_TARGETS = ("random_0.30", "random_0.45", "random_0.60")


@functools.lru_cache(maxsize=None)
def mask_case(name):
    """-> (mask, root, comp, n, size), computed once per process; the arrays are read-only"""
    mask = np.ascontiguousarray(MASKS[name]())
    out = (mask,) + flood_fill(mask)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def random_vote_case(name):
    """a random mask with random targets (outside the mask one half 255, the other 0 .. 12 -- two of them above the
    classes -- SHADOW inside) -> (targets, votes, winner, out, out_plus_one)"""
    mask, _, comp, n, _ = mask_case(name)
    rng = np.random.default_rng(len(name) + int(mask.sum()))
    targets = rng.choice(np.array(list(range(13)) + [255], np.uint8), size=mask.shape, p=[0.5 / 13] * 13 + [0.5])
    targets[mask != 0] = SHADOW
    votes, winner = count_votes(targets, comp, n)
    out = (targets, votes, winner, relabel(targets, comp, winner), relabel(targets, comp, winner, True))
    for a in out:
        a.setflags(write=False)
    return out


# ----------------------------------------------------------------------------------------------------- known answers
def _known(shape, fill, blobs, paint, winners, votes):
    """targets = `fill` with `paint` [(rows, cols, class)] applied, then the blobs [(rows, cols)] set to SHADOW;
    expected: the winners per blob (in row-major order of the blobs' first pixels), some vote counts
    {(blob, class): count}, and the image with every blob that has a winner painted in it"""
    targets = np.full(shape, fill, np.uint8)
    for rows, cols, cls in paint:
        targets[rows, cols] = cls
    for rows, cols in blobs:
        targets[rows, cols] = SHADOW
    out = targets.copy()
    for (rows, cols), win in zip(blobs, winners):
        if win != 255:
            out[rows, cols] = win
    return {"targets": targets, "winners": winners, "votes": votes, "out": out}


def _ring_blob():
    rows, cols = np.nonzero(np.pad(np.zeros((3, 3), bool), 1, constant_values=True))
    return rows + 1, cols + 1


s_ = np.s_
KNOWN = {
    # a 3 x 3 blob in grass with a road along its right side: 32 (component pixel, neighbour) pairs, 9 of them road
    "grass_three_sides_road_one": _known((8, 8), 1, [(s_[2:5], s_[2:5])], [(s_[1:6], 5, 4)], [1],
                                         {(0, 1): 23, (0, 4): 9}),
    # one pixel with two neighbours of class 3 and two of class 2: the smaller class wins the tie
    "tie_goes_to_the_smaller_class": _known((5, 5), 255, [(2, 2)], [(1, 1, 3), (1, 3, 3), (3, 1, 2), (3, 3, 2)], [2],
                                            {(0, 2): 2, (0, 3): 2}),
    # nothing but buildings and unlabelled pixels around: no vote, the blob stays shadow
    "buildings_only": _known((4, 5), BUILDING, [(s_[1:3], s_[1:3])], [(0, s_[0:5], 255)], [255], {(0, BUILDING): 0}),
    # blobs in two corners of the image; class 0 is a winner like any other
    "image_corners": _known((6, 6), 5, [(np.array([0, 0, 1]), np.array([0, 1, 0])), (5, 5)], [(s_[3:6], s_[3:6], 0)],
                            [5, 0], {(0, 5): 7, (1, 0): 3}),
    # a ring around a lit island: the island votes (32 pairs of class 8 against 56 of grass) and keeps its labels
    "ring_around_an_island": _known((7, 7), 1, [_ring_blob()], [(s_[2:5], s_[2:5], 8)], [1], {(0, 1): 56, (0, 8): 32}),
    "two_components_two_winners": _known((6, 12), 0, [(2, 2), (s_[2:4], 8)], [(s_[0:6], s_[6:12], 4)], [0, 4],
                                         {(0, 0): 8, (1, 4): 14}),
    # classes at or above n_classes are no classes: 11 and 200 do not vote, 9 does
    "neighbour_class_out_of_range": _known((5, 5), 255, [(2, 2)], [(1, 1, 11), (1, 2, 200), (1, 3, 9)], [9],
                                           {(0, 9): 1}),
}

def known_case(name):
    case = KNOWN[name]
    plus = case["out"].copy()
    plus[plus != 255] += 1
    return dict(case, out_plus_one=plus)
