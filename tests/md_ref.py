"""The rules of pamnet_md_step_f32 and pamnet_md_init_velocities_f32 (include/pamnet_hip.h) restated in numpy, fp64 -- the
reference of tests/test_md.py.

The generator: Philox4x32-10 (Salmon et al., SC 2011) in uint64 arithmetic.  Key = (low, high 32 bits) of the graph's seed;
counter = (i, step, stream, 0), i the atom's offset in its graph, stream 0 the thermostat, 1 the initial velocities;
u_j = (x_j + 0.5) 2^-32; xi = (r0 cos 2 pi u1, r0 sin 2 pi u1, r1 cos 2 pi u3), r0 = sqrt(-2 ln u0), r1 = sqrt(-2 ln u2).

md_step_ref, per graph g, sums over the free atoms, f = -dE/dpos:
  1. status[g] != 0: g is left alone.
  2. v_n = v + kick_in (dt / 2) f / m.
  3. F2 = sum |f|^2, KE = 1/2 sum m |v_n|^2; ke[g] = KE.  Either not finite: status[g] = 2, nothing else changes.
  4. advance == 0: vel <- v_n, done.
  5. v1 = v_n + (dt / 2) f / m; gamma > 0: v2 = c1 v1 + c2 sqrt(kT / m) xi, c1 = exp(-gamma dt), c2 = sqrt(1 - c1^2); else v2 = v1;
     pos <- pos + (dt / 2)(v1 + v2), vel <- v2.
  6. steps[g] += 1.
fp64 from the fp32 inputs, one rounding to fp32 where pos and vel are stored; fixed atoms are skipped."""
import numpy as np

STATE = ('seed', 'steps', 'status', 'ke')
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
    """counter: four uint32 arrays (or ints), key: two -> the four uint32 output arrays of Philox4x32-10."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k = [np.uint64(int(x) & 0xFFFFFFFF) for x in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return [x.astype(np.uint32) for x in c]


def normals(seed, count, step, stream):
    """The three normals of the atoms 0 .. count - 1 of a graph: float64 [count, 3]."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32((np.arange(count, dtype=np.uint64), int(step) & 0xFFFFFFFF, stream, 0), (seed & 0xFFFFFFFF, seed >> 32))
    u = [(xi.astype(np.float64) + 0.5) * 2.0 ** -32 for xi in x]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    return np.stack([r0 * np.cos(2 * np.pi * u[1]), r0 * np.sin(2 * np.pi * u[1]), r1 * np.cos(2 * np.pi * u[3])], axis=1)


def _free(gptr, g, n, fixed):
    lo, hi = max(int(gptr[g]), 0), min(int(gptr[g + 1]), n)
    hi = max(hi, lo)
    idx = np.arange(lo, hi)
    return lo, hi, idx[~fixed[idx]]


def md_step_ref(pos, vel, dE, gptr, state, dt, kT=0.0, gamma=0.0, mass=None, fixed=None, kick_in=1, advance=1):
    """pos, vel, dE: float32 [n, 3]; gptr: [G + 1]; state: dict of seed (int64; None where gamma is 0), steps, status (int32), ke
    (float64), each [G]; dt, kT, gamma: a float or [G]; mass: float32 [n] or None; fixed: bool [n] or None.  Returns new
    (pos, vel, state); the inputs are not modified."""
    pos, vel = np.array(pos, dtype=np.float32), np.array(vel, dtype=np.float32)
    dE = np.asarray(dE, dtype=np.float32)
    n, G = pos.shape[0], len(gptr) - 1
    st = {k: (None if state[k] is None else np.array(state[k])) for k in STATE}
    assert st['ke'].dtype == np.float64 and st['steps'].dtype == np.int32
    fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool)
    m_all = np.ones(n) if mass is None else np.asarray(mass, dtype=np.float32).astype(np.float64)
    dt, kT, gamma = (np.broadcast_to(np.asarray(x, dtype=np.float64), (G,)) for x in (dt, kT, gamma))
    for g in range(G):
        if st['status'][g] != 0:                                               # 1
            continue
        lo, hi, free = _free(gptr, g, n, fixed)
        h = 0.5 * dt[g]
        with np.errstate(all='ignore'):
            f, v, m = -dE[free].astype(np.float64), vel[free].astype(np.float64), m_all[free][:, None]
            a = f / m
            if kick_in:
                v = v + h * a                                                  # 2
            F2, KE = float((f * f).sum()), 0.5 * float((m * v * v).sum())      # 3
            st['ke'][g] = KE
            if not (np.isfinite(F2) and np.isfinite(KE)):
                st['status'][g] = 2
                continue
            if not advance:                                                    # 4
                vel[free] = v.astype(np.float32)
                continue
            v1 = v + h * a                                                     # 5
            if gamma[g] > 0.0:
                c1 = np.exp(-gamma[g] * dt[g])
                c2 = np.sqrt(1.0 - c1 * c1)
                xi = normals(st['seed'][g], hi - lo, st['steps'][g], 0)[free - lo]
                v2 = c1 * v1 + c2 * np.sqrt(kT[g] / m) * xi
            else:
                v2 = v1
            pos[free] = (pos[free].astype(np.float64) + h * (v1 + v2)).astype(np.float32)
            vel[free] = v2.astype(np.float32)
        st['steps'][g] += 1                                                    # 6
    return pos, vel, st


def init_velocities_ref(vel, gptr, seed, kT, mass=None, fixed=None, remove_com=True, rescale=False):
    """vel: float32 [n, 3] (rows of fixed atoms are kept); seed: int64 [G]; kT: a float or [G].  Returns (vel, ke float64 [G]):
    v = sqrt(kT / m) xi(seed, step 0, stream 1, i); remove_com: v -= sum m v / sum m; rescale: v *= sqrt(dof kT / (2 KE)) where
    dof = 3 n_free - 3 remove_com > 0 and KE > 0; ke is the kinetic energy of v in fp64, before the rounding to fp32."""
    vel = np.array(vel, dtype=np.float32)
    n, G = vel.shape[0], len(gptr) - 1
    fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool)
    m_all = np.ones(n) if mass is None else np.asarray(mass, dtype=np.float32).astype(np.float64)
    kT = np.broadcast_to(np.asarray(kT, dtype=np.float64), (G,))
    ke = np.zeros(G)
    for g in range(G):
        lo, hi, free = _free(gptr, g, n, fixed)
        m = m_all[free][:, None]
        v = np.sqrt(kT[g] / m) * normals(seed[g], hi - lo, 0, 1)[free - lo]
        if remove_com and free.size:
            v = v - (m * v).sum(0) / m.sum()
        KE = 0.5 * float((m * v * v).sum())
        dof = 3 * free.size - (3 if remove_com else 0)
        s = np.sqrt(dof * kT[g] / (2.0 * KE)) if rescale and dof > 0 and KE > 0.0 else 1.0
        vel[free] = (s * v).astype(np.float32)
        ke[g] = s * s * KE
    return vel, ke
