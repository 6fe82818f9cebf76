"""CPU restatement of the particle mover (mg3d_particle_push(_device), mg3d_particle_counts; include/mg3d.h, "Particles"):
numpy with the library's operands in the library's order, step by step, and exact integers for the table of fates.  Built
on tests/_particle_ref.py: its locator and its sample are the mover's.

axes is the mask of periodic axes, faces the mask of Neumann faces.  Positions and velocities are (M, 3).  Also the
particles, fields and masks of the push tests, so that the host test can hold the seeds of the GPU test to their coverage.
Test infrastructure only."""
import numpy as np

import _field_ref as FR
import _particle_ref as PR

ALIVE, FACE, INVALID, SLOTS = 0, 256, 262, 263
LABELS = (3, 200)


def constants(N, h, dt, scale=-1.0, accel=(0.0, 0.0, 0.0), drag=0.0):
    """the host constants in the header's order: (cs, gdt (3,), inv, n1, xper, xhi), all Python / numpy float64"""
    h, dt, scale, drag = np.float64(h), np.float64(dt), np.float64(scale), np.float64(drag)
    cs = scale * (np.float64(0.5) / h)
    gdt = np.array([dt * np.float64(a) for a in accel], dtype=np.float64)
    inv = np.float64(1.0) / (np.float64(1.0) + drag * dt)
    n1 = np.float64(N - 1)
    xper = n1 * h
    xhi = xper
    while xhi / h > n1:
        xhi = np.nextafter(xhi, np.float64(0.0))
    return cs, gdt, inv, n1, xper, xhi


def new_table():
    return np.zeros(SLOTS, dtype=np.uint64)


def new_events():
    """what happened at the walls, per axis: reflections at the low and high face, wraps from below and from above"""
    return {k: [0, 0, 0] for k in ("reflect_lo", "reflect_hi", "wrap_lo", "wrap_hi")}


def push(u, mask, xyz, vel, qm, fate, h, axes, faces, dt, scale=-1.0, accel=(0.0, 0.0, 0.0), drag=0.0, table=None,
         events=None):
    """one push: new arrays (xyz float64, vel in vel's dtype, fate int32).  u (N, N, N); mask (N, N, N) uint8 or None; qm
    (M,) or a scalar, float64 or float32; fate (M,) int32.  table (new_table()) receives the transitions, events
    (new_events()) what the walls did."""
    N = u.shape[0]
    xyz = np.array(xyz, dtype=np.float64)
    vel = np.array(vel)
    assert vel.dtype in (np.float64, np.float32) and xyz.shape == vel.shape and xyz.shape[1] == 3
    fate = np.array(fate, dtype=np.int32)
    M = xyz.shape[0]
    qm = np.broadcast_to(np.asarray(qm), (M,)).astype(np.float64)  # (a float32 widens exactly)
    cs, gdt, inv, n1, xper, xhi = constants(N, h, dt, scale, accel, drag)
    dt, h = np.float64(dt), np.float64(h)
    alive = np.nonzero(fate == ALIVE)[0]
    if alive.size == 0:
        return xyz, vel, fate
    x0 = xyz[alive]
    new_fate = np.zeros(alive.size, dtype=np.int32)
    with np.errstate(all="ignore"):
        # 1 locate x0
        t = x0 / h
        finite = (np.isfinite(x0) & np.isfinite(t)).all(axis=1)
        inside = np.ones(alive.size, dtype=bool)
        first = np.full(alive.size, -1, dtype=np.int32)
        for ax in range(3):
            here = PR.locate_axis(x0[:, ax], h, N, FR.per(axes, ax))[0]
            inside &= here
            out_here = ~here & (first < 0)
            first = np.where(out_here, 2 * ax + np.where(t[:, ax] < 0.0, 0, 1), first).astype(np.int32)
        new_fate = np.where(~inside, np.where(finite, FACE + first, INVALID), new_fate).astype(np.int32)
        go = np.nonzero(inside)[0]
        if go.size:
            xg = x0[go]
            # 2 gather: the sample's gradient at x0 with this scale
            E = PR.sample(u, xg, h, axes, faces, scale)[1]
            # 3 kick and drift
            k = qm[alive][go] * dt
            v0 = vel[alive][go].astype(np.float64)
            v1 = (v0 + ((k[:, None] * E) + gdt[None, :])) * inv
            x1 = xg + (dt * v1)
            ok = np.isfinite(k) & np.isfinite(v1).all(axis=1) & np.isfinite(x1).all(axis=1)
            f = np.where(ok, ALIVE, INVALID).astype(np.int32)
            # 4 walls
            for ax in range(3):
                tt = x1[:, ax] / h
                xa, va = x1[:, ax].copy(), v1[:, ax].copy()
                if FR.per(axes, ax):
                    lo, hi = ok & (tt < 0.0), ok & ~(tt < 0.0) & (tt >= n1)
                    xa = np.where(lo, xa + xper, np.where(hi, xa - xper, xa))
                    if events is not None:
                        events["wrap_lo"][ax] += int(lo.sum())
                        events["wrap_hi"][ax] += int(hi.sum())
                else:
                    lo, hi = ok & (tt < 0.0), ok & ~(tt < 0.0) & (tt > n1)
                    if FR.neu(faces, ax, 0):
                        xa, va = np.where(lo, -xa, xa), np.where(lo, -va, va)
                        if events is not None:
                            events["reflect_lo"][ax] += int(lo.sum())
                    else:
                        f = np.where(lo & (f == ALIVE), FACE + 2 * ax, f).astype(np.int32)
                    if FR.neu(faces, ax, 1):
                        xa, va = np.where(hi, xhi - (xa - xhi), xa), np.where(hi, -va, va)
                        if events is not None:
                            events["reflect_hi"][ax] += int(hi.sum())
                    else:
                        f = np.where(hi & (f == ALIVE), FACE + 2 * ax + 1, f).astype(np.int32)
                x1[:, ax], v1[:, ax] = xa, va
            # 5 conductors: the byte at the node nearest to the final position, where that is inside
            if mask is not None:
                there = np.ones(go.size, dtype=bool)
                node = []
                for ax in range(3):
                    here, c, _, w1 = PR.locate_axis(x1[:, ax], h, N, FR.per(axes, ax))
                    there &= here
                    n = c + (w1 >= 0.5)
                    node.append(PR.source(n, N, FR.per(axes, ax)))
                b = np.asarray(mask, dtype=np.uint8).reshape(N, N, N)[tuple(node)].astype(np.int32)
                f = np.where(there & (f == ALIVE) & (b != 0), b, f).astype(np.int32)
            # 6 stores (a particle that step 3 found not finite keeps its position and velocity)
            rows = alive[go][ok]
            xyz[rows] = x1[ok]
            vel[rows] = v1[ok].astype(vel.dtype)
            new_fate[go] = f
    fate[alive] = new_fate
    if table is not None:
        table += np.bincount(new_fate[new_fate != ALIVE], minlength=SLOTS).astype(np.uint64)
    return xyz, vel, fate


# ----------------------------------------------------------------------------------------------------------- test cases
# (periodic axes, Neumann faces), the sets of tests/test_gpu_particles.py
BCS = {"dirichlet": (0, 0), "per7": (7, 0), "per4_f15": (4, 15), "f63": (0, 63), "f22": (0, 22), "f25": (0, 0b011001)}
DT = 0.125
PAST_CAP_COUNT = 2048 * 256 + 259  # tests/test_particle_ref_host.py holds it to the grid cap
# (N, boundary set, seeded particles beside the edge points, with a mask, pushes in sequence).  The case past the grid cap
# takes three pushes: twenty of half a million particles would take the restatement a minute.
CASES = ([(5, bc, 257, n % 2 == 0, 20) for n, bc in enumerate(BCS)] + [(17, bc, 255, n % 2 == 1, 20) for n, bc in enumerate(BCS)]
         + [(37, "dirichlet", 4099, True, 20), (37, "per7", 256, False, 20), (37, "f25", 1, True, 20),
            (65, "f63", 256, True, 20), (65, "per4_f15", 1, False, 20), (65, "f22", 4099, False, 20),
            (65, "per7", 4099, True, 20), (17, "per4_f15", PAST_CAP_COUNT, True, 3)])


def spacing(N, grid_length=1.0):
    """h of a box of side grid_length, as the library forms it"""
    return grid_length / (N - 1)


def bodies(N):
    """two conductors: a block labelled 3 and a plate labelled 200"""
    m = np.zeros((N, N, N), dtype=np.uint8)
    a, w = max(1, N // 6), max(1, N // 4)
    m[a:a + w, a:a + w, a:a + w] = LABELS[0]
    p, th = (2 * N) // 3, max(1, N // 16)
    m[p:p + th, N // 4:N - N // 4, N // 4:N - N // 4] = LABELS[1]
    return m


def particles(N, h, axes, count, seed, nodes=False):
    """(xyz, vel, qm) of a case: `count` seeded points inside the box and then the edge points of the sample's tests (a
    count of 1: the one point alone), speeds up to 1.5 h per step on each axis -- a quarter of the particles fifty times
    slower, so that some stay --, q/m for kicks of up to a hundredth of a spacing against a field of size 1/h; one velocity
    and one q/m that are not finite.  Everything is written in units of h (the box's own: h carries the grid length) and
    DT.  nodes: PR.node_points_all(N, h) behind the edge points"""
    rng = np.random.default_rng(seed)
    xyz = PR.box_points(N, h, count, seed)
    if count > 1:
        xyz = np.concatenate([xyz, PR.edge_points(N, h, axes)] + ([PR.node_points_all(N, h)] if nodes else []))
    M = xyz.shape[0]
    vel = rng.uniform(-1.5, 1.5, (M, 3)) * (h / DT)
    vel[rng.uniform(size=M) < 0.25] *= 0.02
    qm = rng.uniform(-1.0, 1.0, M) * (0.01 * h * h / (DT * DT))
    if M > 20:
        vel[7, 1] = np.nan
        qm[9] = np.inf
    return xyz, vel, qm


def field(N, seed):
    """random u at every point, Dirichlet faces and periodic duplicates too"""
    return np.random.default_rng(seed).uniform(-1, 1, (N, N, N))


def case_data(N, bc, count, with_mask, grid_length=1.0, nodes=False):
    """(u, mask or None, xyz, vel, qm, accel, drag) of a case of CASES, on a box of side grid_length (velocities, q/m and
    accel are in units of h and DT: they carry over)"""
    axes, faces = BCS[bc]
    h = spacing(N, grid_length)
    u = field(N, 1000 * N + axes * 64 + faces)
    xyz, vel, qm = particles(N, h, axes, count, 7 * N + count + axes + faces, nodes)
    accel = (0.0, 0.0, -0.002 * h / (DT * DT))
    return u, (bodies(N) if with_mask else None), xyz, vel, qm, accel, 0.25


def run_case(N, bc, count, with_mask, pushes, events=None, grid_length=1.0, nodes=False, vel_dtype=np.float64):
    """the restatement's states after each push: [(xyz, vel, fate, table copy)]"""
    axes, faces = BCS[bc]
    u, mask, xyz, vel, qm, accel, drag = case_data(N, bc, count, with_mask, grid_length, nodes)
    with np.errstate(over="ignore", invalid="ignore"):
        vel = vel.astype(vel_dtype)
    fate = np.zeros(xyz.shape[0], dtype=np.int32)
    table = new_table()
    out = []
    h = spacing(N, grid_length)
    for _ in range(pushes):
        xyz, vel, fate = push(u, mask, xyz, vel, qm, fate, h, axes, faces, DT, -1.0, accel, drag, table, events)
        out.append((xyz, vel, fate, table.copy()))
    return out
