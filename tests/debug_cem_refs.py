"""numpy restatement of the planner's --debug_cem sheet (reference src/cem/cem.py:140-175, push/cem.py:183-239; the layout
rac_cem_rollout_sheet writes), twice: `sheet_vectorised` with array operations, `sheet_loops` pixel by pixel.  The two are
compared in tests/test_debug_cem_host.py; the GPU tests compare the kernel with `sheet_vectorised`.

frames  (n, T, 3, H, W) float32: every candidate's predicted frames (planar, values in [0, 1])
rows    the candidate shown in each row block (any order, repeats allowed)
start   (H, W, 3) uint8;  goals (G, H, W, 3) uint8;  goal_masks None or (G, H, W), != 0 is robot
->      (T+1, R*H, 3*W, 3) uint8:  sheet 0, every block: [zeros | start | goals[0]] (never masked)
                                   sheet t+1, block r:   [zeros | u8(frames[rows[r], t]) | goals[min(t, G-1)], robot pixels 0]
"""
import numpy as np


def u8(x):
    """The fp32 product 255 * x truncated toward zero: what `np.uint8(255 * obs)` gives for float32 obs in [0, 1]."""
    return (np.float32(255) * np.asarray(x, np.float32)).astype(np.uint8)


def sheet_vectorised(frames, rows, start, goals, goal_masks=None):
    frames, goals = np.asarray(frames, np.float32), np.asarray(goals, np.uint8)
    n, T, _, H, W = frames.shape
    R, G = len(rows), len(goals)
    out = np.zeros((T + 1, R, H, 3, W, 3), np.uint8)  # (sheet, block, y, panel, x, channel)
    out[0, :, :, 1] = np.asarray(start, np.uint8)
    out[0, :, :, 2] = goals[0]
    out[1:, :, :, 1] = u8(frames[np.asarray(rows)]).transpose(1, 0, 3, 4, 2)  # (R, T, 3, H, W) -> (T, R, H, W, 3)
    g = np.minimum(np.arange(T), G - 1)
    shown = goals[g].copy()
    if goal_masks is not None:
        shown[np.asarray(goal_masks)[g] != 0] = 0
    out[1:, :, :, 2] = shown[:, None]
    return out.reshape(T + 1, R * H, 3 * W, 3)


def sheet_loops(frames, rows, start, goals, goal_masks=None):
    n, T, _, H, W = np.shape(frames)
    R, G = len(rows), len(goals)
    out = np.full((T + 1, R * H, 3 * W, 3), 77, np.uint8)  # every byte must be written below
    for s in range(T + 1):
        for r in range(R):
            for y in range(H):
                for x in range(W):
                    for c in range(3):
                        out[s, r * H + y, x, c] = 0
                        if s == 0:
                            out[s, r * H + y, W + x, c] = start[y][x][c]
                            out[s, r * H + y, 2 * W + x, c] = goals[0][y][x][c]
                        else:
                            t = s - 1
                            g = t if t < G else G - 1
                            v = np.float32(255) * np.float32(frames[rows[r]][t][c][y][x])
                            out[s, r * H + y, W + x, c] = int(v)
                            robot = goal_masks is not None and goal_masks[g][y][x] != 0
                            out[s, r * H + y, 2 * W + x, c] = 0 if robot else goals[g][y][x][c]
    return out


def planted_values():
    """Frame values at which a wrong rounding rule shows: 0, 1, the float below 1, every k / 255 with its two float32
    neighbours, and 0.5 / 255."""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    vals = np.concatenate([[0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), np.float32(0.5) / np.float32(255)],
                           k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2))]).astype(np.float32)
    return np.clip(vals, 0, 1)


def random_problem(seed, n, T, H, W, G, with_mask):
    """Seeded frames (uniform in [0, 1], the planted values scattered over the last candidate's), start, goals and goal
    masks (the first goal's mask all robot)."""
    g = np.random.Generator(np.random.Philox(key=[seed, n * 1000 + T * 100 + G]))
    frames = g.random((n, T, 3, H, W), dtype=np.float32)
    flat = frames[n - 1].reshape(-1)  # a view: the last candidate carries the planted values (the tests always show it)
    pv = g.permutation(planted_values())  # (frames smaller than the list take a seeded part of it)
    pos = g.permutation(flat.size)[:min(len(pv), flat.size // 2)]
    flat[pos] = pv[:len(pos)]
    start = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    goals = g.integers(0, 256, (G, H, W, 3), dtype=np.uint8)
    masks = None
    if with_mask:
        masks = (g.random((G, H, W)) < 0.3).astype(np.uint8) * g.integers(1, 256, (G, H, W), dtype=np.uint8)
        masks[0] = 1
    return frames, start, goals, masks
