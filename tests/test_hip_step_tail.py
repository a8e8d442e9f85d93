"""The small kernels around the layer stack -- csrc/basis.hip (Bessel / spherical bases, attention fusion, pooling),
csrc/embed.hip (the input stage) and csrc/optim.hip (Adam + EMA) -- on the far side of their grid caps and unrolled loops,
against plain fp64 statements of the same operations (oracle/pamnet_oracle.py, or a few lines of torch / numpy here).

Each of these kernels has a capped grid or an unrolled strided loop, and the rest of the suite stays where every thread or
workgroup runs its loop body once.  The sizes below are derived from the caps (restated in the table, guarded by CPU tests
that read the sources, so that a retuned cap moves the sizes or fails with a message):

    pool_kernel                  one wave per graph; `for (; v + 192 < end; v += 256)` unrolled four ways, then a 64-stride tail:
                                 graphs of 192 / 193, 255 / 256 / 257, 448 / 449, 511 / 512 / 513 and 2200 nodes
    rbf_bwd_*partial_kernel      2048 workgroups x 16 row slots: above 32 768 edges a thread strides; 32 769, 65 541, 100 003
    sbf_combine_kernel           64-row tiles, a thread walks rows r0, r0 + 6, ...: ragged last tile, repeated sources
    launch_multi (embed.hip)     by cost up to 4 * 512 tiles, beyond it two tiles per workgroup up to 256: 2048 / 2049 tiles
    adam_ema_*kernel             4096 workgroups x 256 float4: above 4 194 304 floats the loop runs a second pass

Bounds.  Pooling of exact half-integers: bit for bit.  Fusion + pooling in general: max(5e-6, 2 * err32), whole tensors and
every graph against its own sum of absolute terms.  Gradients summed over all m rows (the Bessel frequencies):
max(1e-5, 4 * err32), the bound of test_hip_narrow_walk.py.  The spherical-basis combine rounds one fp64 product:
|got - ref| <= 2^-23 |ref| + 1e-12.  The input stage: the protocol and floors of test_hip_fused.py (its own test bodies, run
at these sizes).  Adam: RTOL = ATOL = 1e-6 of test_hip_trainer_groups.py.  err32 is always the error of the same formula in
plain fp32 torch on the same inputs against the same fp64 reference.  Measured figures: profiles/step_tail_errors.txt (each
check prints its line; run with -s to collect them)."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import maxnorm_err

# ---- the caps and loop shapes of the three sources, restated ----------------------------------------------------------
RBF_BWD_BLOCKS = 2048                     # basis.hip, pamnet_rbf_bwd_f32 / _env_f32: workgroups of the partial kernel
RBF_ROW_SLOTS = 16                        # ... row slots per workgroup (256 threads / 16 frequencies)
RBF_FINAL_SLICES = 64                     # rbf_bwd_final_kernel: slices of the partials (2048 / 64 = 32 per slice)
POOL_GUARD, POOL_STEP, WAVE = 192, 256, 64   # pool_kernel: `for (; v + 192 < end; v += 256)`, then `v += 64`
POOL_WAVES = 4                            # waves (graphs) per pooling workgroup
SBF_ROWS = 64                             # rows per workgroup of the combine kernels
SBF_ROW_STEP = 6                          # sbf_combine_kernel: 252 threads = 6 rows x 42 columns, r += 6
TR = 64                                   # embed.hip: rows per tile
FWD_CAP, BWD_SLOTS, BWD_BIG_CAP = 1024, 512, 256
PLAN_SWITCH_TILES = 4 * BWD_SLOTS         # `all_tiles <= 4 * BWD_SLOTS`: dealt by cost; above: two tiles per workgroup up to 256
TILE_COST = {'C42_TWO': 5, 'C42': 3, 'C16_RBF': 2, 'C16_DX': 2, 'C16': 1, 'C18': 1}
TYPE_BLOCKS, TYPE_ROWS_PER_BLOCK = 64, 128   # type_rows_core.h blocks_for_rows: the type-table job's workgroups
ADAM_BLOCKS = 4096                        # optim.hip: `if (blocks > 4096) blocks = 4096`, 256 threads, one float4 each

RBF_CAP_ROWS = RBF_BWD_BLOCKS * RBF_ROW_SLOTS          # 32 768: above it a thread strides over several edges
ADAM_CAP = ADAM_BLOCKS * 256 * 4                       # 4 194 304 floats: above it the grid-stride loop runs again

POOL_SIZES = [0, 1, 63, 64, 65, 192, 193, 255, 256, 257, 448, 449, 511, 512, 513, 2200, 0, 0]
RBF_ROWS = [0, 1, 15, 16, 17, RBF_CAP_ROWS, RBF_CAP_ROWS + 1, 2 * RBF_CAP_ROWS + 5, 100003]
SBF_M = [1, 63, 64, 65, 4099]
SBF_EDGES = [1, 7, 300]
INPUT_SIZES = [(300, 118720, 12000, 600), (300, 118721, 12000, 600)]      # (e_l, e_g, tp, n): 2048 and 2049 tiles (types_two)
EMBED_ROWS = PLAN_SWITCH_TILES * TR + 1                                   # 131 073: one job of 2049 tiles
ADAM_N_PLAIN = ADAM_CAP + 2052
ADAM_N_GROUPS = ADAM_CAP + 64 * 33

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'physics-aware-multiplex-gnn_amd', 'csrc')


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _count(text, name, pattern, want):
    found = re.findall(pattern, text)
    assert len(found) == want, ('%s: expected %d match(es) of %r, found %d -- the cap or loop was reshaped: restate it in the '
                                'table of tests/test_hip_step_tail.py, so that its sizes move with it' % (name, want, pattern, len(found)))
    return found


# ---- CPU guards: the table against the sources --------------------------------------------------------------------------
def check_basis(text):
    cap = _count(text, 'basis.hip', r'int nblocks = \(int\)\(m > 0 \? \(ceil_div\(m, (\d+)\) < (\d+) \? ceil_div\(m, (\d+)\) : (\d+)\) : 0\);', 2)
    for a, b, c, d in cap:                                       # pamnet_rbf_bwd_f32 and pamnet_rbf_bwd_env_f32
        assert (int(a), int(b), int(c), int(d)) == (RBF_ROW_SLOTS, RBF_BWD_BLOCKS, RBF_ROW_SLOTS, RBF_BWD_BLOCKS), cap
    stride = _count(text, 'basis.hip', r'for \(int64_t e = \(int64_t\)blockIdx\.x \* (\d+) \+ slot; e < m; e \+= \(int64_t\)gridDim\.x \* (\d+)\)', 2)
    assert all((int(a), int(b)) == (RBF_ROW_SLOTS, RBF_ROW_SLOTS) for a, b in stride), stride
    fin = _count(text, 'basis.hip', r'for \(int b = sl; b < nblocks; b \+= (\d+)\) s \+= partial\[b \* 16 \+ n\];', 1)
    assert int(fin[0]) == RBF_FINAL_SLICES
    loop = _count(text, 'basis.hip', r'for \(; v \+ (\d+) < end; v \+= (\d+)\) \{', 1)
    assert (int(loop[0][0]), int(loop[0][1])) == (POOL_GUARD, POOL_STEP), loop
    tail = _count(text, 'basis.hip', r'for \(; v < end; v \+= (\d+)\) s0 \+= node_out\[v\];', 1)
    assert int(tail[0]) == WAVE
    _count(text, 'basis.hip', r'hipLaunchKernelGGL\(pool_kernel, dim3\(blocks_for\(n_graphs, %d\)\), dim3\(256\)' % POOL_WAVES, 1)
    rows = _count(text, 'basis.hip', r'constexpr int SBF_ROWS = (\d+);', 1)
    assert int(rows[0]) == SBF_ROWS
    step = _count(text, 'basis.hip', r'for \(int r = r0; r < rows; r \+= (\d+), out \+= 252\)', 1)
    assert int(step[0]) == SBF_ROW_STEP


def check_embed(text, type_rows_text):
    assert int(_count(text, 'embed.hip', r'constexpr int TR = (\d+);', 1)[0]) == TR
    caps = _count(text, 'embed.hip', r'constexpr int FWD_CAP = (\d+), BWD_SLOTS = (\d+);', 1)[0]
    assert (int(caps[0]), int(caps[1])) == (FWD_CAP, BWD_SLOTS), caps
    big = _count(text, 'embed.hip', r'#ifndef EMBED_BWD_BIG_CAP\n#define EMBED_BWD_BIG_CAP (\d+)', 1)
    assert int(big[0]) == BWD_BIG_CAP
    sw = _count(text, 'embed.hip', r'const bool by_cost = all_tiles <= (\d+) \* BWD_SLOTS;', 1)
    assert int(sw[0]) * BWD_SLOTS == PLAN_SWITCH_TILES
    # the deal itself, as launch_plan() below restates it
    _count(text, 'embed.hip', r'inline int bwd_grid_max\(int64_t rows\) \{ return grid_for\(rows, BWD_SLOTS\); \}', 1)
    _count(text, 'embed.hip', r'int64_t want = grid_for\(\(J\.job\[j\]\.rows \+ 1\) / 2, EMBED_BWD_BIG_CAP\);', 1)
    _count(text, 'embed.hip', r'if \(by_cost\) want = total > 0 \? \(tiles \* tile_cost\(J\.job\[j\]\.code\) \* budget \+ total - 1\) / total : 1;', 1)
    _count(text, 'embed.hip', r'const int64_t budget = BWD_SLOTS - J\.types\.nblk > 64 \? BWD_SLOTS - J\.types\.nblk : 64;', 1)
    _count(text, 'embed.hip', r'inline int tile_cost\(int code\) \{ return code == C42_TWO \? 5 : \(code == C42 \? 3 : '
                              r'\(code == C16_RBF \|\| code == C16_DX \? 2 : 1\)\); \}', 1)
    _count(text, 'embed.hip', r'for \(int64_t tile = bid; tile < ntiles; tile \+= jb\.nblk\) \{', 2)          # forward and backward walk
    _count(text, 'embed.hip', r'pre\[i\] = \(t < ntiles && g < rows\) \? ldg4\(gout, g, DOUT, c4p\) : f4zero\(\);', 1)
    _count(text, 'embed.hip', r'prefetch\(tile \+ jb\.nblk\);', 1)
    tb = _count(type_rows_text, 'type_rows_core.h', r'constexpr int TYPE_MAX = \d+, TYPE_BLOCKS = (\d+);', 1)
    assert int(tb[0]) == TYPE_BLOCKS
    _count(type_rows_text, 'type_rows_core.h', r'int64_t blocks = \(n \+ %d\) / %d;' % (TYPE_ROWS_PER_BLOCK - 1, TYPE_ROWS_PER_BLOCK), 1)


def check_optim(text):
    caps = _count(text, 'optim.hip', r'if \(blocks > (\d+)\) blocks = (\d+);', 2)                 # adam_launch and the groups entry
    assert all((int(a), int(b)) == (ADAM_BLOCKS, ADAM_BLOCKS) for a, b in caps), caps
    _count(text, 'optim.hip', r'int64_t blocks = ceil_div\(n4, 256\);', 2)
    _count(text, 'optim.hip', r'for \(int64_t i = \(int64_t\)blockIdx\.x \* 256 \+ threadIdx\.x; i < n4; i \+= \(int64_t\)gridDim\.x \* 256\) \{', 2)
    _count(text, 'optim.hip', r'const int grp = chunk_group\[i >> 4\] & \(MAX_GROUPS - 1\);', 1)


def test_table_matches_the_sources():
    check_basis(_source('basis.hip'))
    check_embed(_source('embed.hip'), _source('type_rows_core.h'))
    check_optim(_source('optim.hip'))


def test_guards_notice_a_reshaped_cap():
    """The guards fail on a source whose cap or loop differs (texts edited here, never compiled)."""
    for name, check, old, new in (
            ('basis.hip', check_basis, 'v + 192 < end; v += 256', 'v + 448 < end; v += 512'),
            ('basis.hip', check_basis, 'ceil_div(m, 16) : 2048) : 0);\n    if (nblocks > 0) {\n        hipLaunchKernelGGL(rbf_bwd_partial_kernel',
             'ceil_div(m, 16) : 4096) : 0);\n    if (nblocks > 0) {\n        hipLaunchKernelGGL(rbf_bwd_partial_kernel'),
            ('basis.hip', check_basis, 'constexpr int SBF_ROWS = 64;', 'constexpr int SBF_ROWS = 128;'),
            ('optim.hip', check_optim, 'if (blocks > 4096) blocks = 4096;\n    if (shadow)', 'if (blocks > 8192) blocks = 8192;\n    if (shadow)'),
            ('embed.hip', lambda t: check_embed(t, _source('type_rows_core.h')), 'all_tiles <= 4 * BWD_SLOTS', 'all_tiles <= 8 * BWD_SLOTS'),
            ('embed.hip', lambda t: check_embed(t, _source('type_rows_core.h')), '#define EMBED_BWD_BIG_CAP 256', '#define EMBED_BWD_BIG_CAP 512')):
        text = _source(name)
        assert text.count(old) == 1, (name, old)
        with pytest.raises(AssertionError):
            check(text.replace(old, new))


# ---- pool_kernel's walk, restated: which nodes a lane adds, in which loop ------------------------------------------------
def pool_walk(size, guard=POOL_GUARD):
    """(visits per node offset [size + 256], unrolled passes of lane 0, tail passes of lane 0) of one wave over a graph of
    `size` nodes; guard: the constant of the unrolled loop's bound (a parameter so that the test can show what a wrong one
    does -- offsets >= size belong to the next graph)."""
    seen = np.zeros(size + POOL_STEP, np.int64)
    passes = tails = 0
    for lane in range(WAVE):
        v = lane
        while v + guard < size:
            for k in range(0, POOL_STEP, WAVE):
                seen[v + k] += 1
            v += POOL_STEP
            passes += lane == 0
        while v < size:
            seen[v] += 1
            v += WAVE
            tails += lane == 0
    return seen, passes, tails


def test_pool_sizes_reach_the_unrolled_loop_and_its_hand_over():
    assert len(POOL_SIZES) % POOL_WAVES != 0 and POOL_SIZES[0] == 0 and POOL_SIZES[-2:] == [0, 0] and sum(POOL_SIZES) == 5979
    state = {}
    for size in sorted(set(POOL_SIZES)):
        seen, passes, tails = pool_walk(size)
        assert (seen[:size] == 1).all() and (seen[size:] == 0).all(), size
        state[size] = (passes, tails)
    g, s = POOL_GUARD, POOL_STEP
    assert state[g] == (0, 3) and state[g + 1] == (1, 0)                 # the first size at which the unrolled loop runs
    assert state[s - 1] == (1, 0) and state[s] == (1, 0) and state[s + 1] == (1, 1)       # hand-over to the tail: lane 0 alone
    assert state[s + g] == (1, 3) and state[s + g + 1] == (2, 0)
    assert state[2 * s - 1] == (2, 0) and state[2 * s] == (2, 0) and state[2 * s + 1] == (2, 1)
    assert state[2200] == (8, 3) and state[63] == (0, 1) and state[65] == (0, 2)
    # a loop bound without the + 192 adds nodes of the next graph at every size that is no multiple of 256: the exact-count
    # test below cannot pass with it
    for size in (1, 63, 193, 257, 449, 513, 2200):
        seen, _, _ = pool_walk(size, guard=0)
        assert seen[size:].sum() > 0, size


def _pool_graph(sizes, dev, with_sign, gen):
    n = int(sum(sizes))
    gptr = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32))
    node_graph = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(torch.int32)
    sign = torch.where(torch.rand(n, generator=gen) > 0.5, 1.0, -1.0) if with_sign else None
    g = types.SimpleNamespace(n_graphs=len(sizes), gptr=gptr.to(dev), node_graph=node_graph.to(dev),
                              sign=None if sign is None else sign.to(dev))
    return g, node_graph.long(), sign


def _pool_exact_inputs(sizes):
    """Small random integers in outs, atts[0] == atts[1]: both softmax weights are exactly 0.5, node_out an exact
    half-integer.  Returns (outs [2, n], atts [2, n], sign [n]) on the CPU and twice node_out without its sign, int64."""
    gen = torch.Generator().manual_seed(1000 + len(sizes))
    n = int(sum(sizes))
    outs = torch.randint(-8, 9, (2, n), generator=gen).float()
    att = torch.randn(1, n, generator=gen)
    sign = torch.where(torch.rand(n, generator=gen) > 0.5, 1.0, -1.0)
    return outs, torch.cat([att, att], 0).contiguous(), sign, (outs[0] + outs[1]).long()


@pytest.mark.parametrize('sizes', [POOL_SIZES, [2200]], ids=['18-graphs', 'one-graph'])
def test_pool_exact_sums_fit_fp32(sizes):
    """Every sum and partial sum of the half-integers stays below 2^23 in magnitude: fp32 addition of them is exact in any order."""
    outs, atts, sign, twice = _pool_exact_inputs(sizes)
    assert torch.equal(atts[0], atts[1]) and torch.equal(outs, outs.round())
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    for b in range(len(sizes)):
        assert 0.5 * float(twice[ptr[b]:ptr[b + 1]].abs().sum()) < 2.0 ** 23        # bounds every partial sum, signed or not
    assert int(twice.abs().max()) > 0


# ---- launch_multi's deal of backward workgroups, restated -------------------------------------------------------------
def _grid_for(rows, cap):
    tiles = -(-rows // TR)
    return max(1, min(tiles, cap))


def launch_plan(jobs, type_rows=None):
    """jobs: [(code, rows)] of one backward launch, type_rows: rows of the type-table job or None.  Returns (by_cost,
    [workgroups per job]) as launch_multi of csrc/embed.hip deals them."""
    tiles = [-(-rows // TR) for _, rows in jobs]
    types_nblk = 0 if type_rows is None else max(1, min((type_rows + TYPE_ROWS_PER_BLOCK - 1) // TYPE_ROWS_PER_BLOCK, TYPE_BLOCKS))
    all_tiles = sum(tiles)
    total = sum(t * TILE_COST[code] for t, (code, _) in zip(tiles, jobs))
    by_cost = all_tiles <= PLAN_SWITCH_TILES
    budget = max(BWD_SLOTS - types_nblk, 64)
    nblk = []
    for t, (code, rows) in zip(tiles, jobs):
        want = _grid_for((rows + 1) // 2, BWD_BIG_CAP)
        if by_cost:
            want = (t * TILE_COST[code] * budget + total - 1) // total if total > 0 else 1
        nblk.append(min(max(want, 1), _grid_for(rows, BWD_SLOTS)))
    return by_cost, nblk


def _walk(rows, nblk):
    """(fewest, most tiles a workgroup of the job walks, workgroup that holds the last tile, its pass index there)."""
    tiles = -(-rows // TR)
    return tiles // nblk, -(-tiles // nblk), (tiles - 1) % nblk, (tiles - 1) // nblk


def _input_jobs(sizes, variant):
    e_l, e_g, tp, n = sizes
    jobs = [('C16_RBF', e_l), ('C16_RBF', e_g), ('C42_TWO' if variant != 'types_one' else 'C42', tp)]
    if variant == 'init18_two':
        return jobs + [('C18', n)], None
    return jobs, n


def test_input_stage_sizes_take_the_plans_they_are_meant_for():
    small, large = INPUT_SIZES
    tiles = lambda jobs: sum(-(-r // TR) for _, r in jobs)
    # types_two: three jobs, one tile apart around the switch
    js, tr = _input_jobs(small, 'types_two')
    jl, _ = _input_jobs(large, 'types_two')
    assert tiles(js) == PLAN_SWITCH_TILES and tiles(jl) == PLAN_SWITCH_TILES + 1
    by_cost, nblk = launch_plan(js, tr)
    assert by_cost and nblk == [2, 404, 103] and _walk(small[1], nblk[1])[:2] == (4, 5)
    by_cost, nblk = launch_plan(jl, tr)
    assert not by_cost and nblk == [3, BWD_BIG_CAP, 94]
    lo, hi, wg, at = _walk(large[1], nblk[1])
    assert lo >= 7 and hi == 8 and large[1] % TR == 1                 # the Bessel job: 7 to 8 tiles per workgroup, a 1-row last tile
    assert at == hi - 1 >= 7 and 0 < wg < nblk[1] - 1                 # ... which is its workgroup's last pass, mid-grid
    # init18_two: the 18-wide job's ten tiles put BOTH sizes beyond the switch (2058 / 2059 tiles): four jobs in the large
    # plan, the 18-wide one with two tiles per workgroup
    for sizes in INPUT_SIZES:
        j4, tr4 = _input_jobs(sizes, 'init18_two')
        by_cost, nblk = launch_plan(j4, tr4)
        assert tr4 is None and tiles(j4) == tiles(_input_jobs(sizes, 'types_two')[0]) + 10 and not by_cost
        assert nblk == [3, BWD_BIG_CAP, 94, 5] and _walk(sizes[1], nblk[1])[0] >= 7
    # one job alone, one tile beyond the switch: 256 workgroups of 8 tiles, the first a ninth of one row
    assert EMBED_ROWS == 131073 and -(-EMBED_ROWS // TR) == PLAN_SWITCH_TILES + 1
    for code in ('C16_DX', 'C42_TWO'):                                # test_embed_layers' rbf16 (dx written) and sbf42_kind
        by_cost, nblk = launch_plan([(code, EMBED_ROWS)])
        assert not by_cost and nblk == [BWD_BIG_CAP] and _walk(EMBED_ROWS, nblk[0]) == (8, 9, 0, 8)
        assert launch_plan([(code, EMBED_ROWS - 1)]) == (True, [BWD_SLOTS])
    # the largest launches of test_hip_fused.py stay below the switch (what this file adds)
    assert launch_plan(*_input_jobs((300, 70001, 40000, 513), 'types_two'))[0] and launch_plan([('C16_DX', 40001)])[0]


def test_prefetch_walk_restated():
    """The carried prefetch of embed_bwd_body on the CPU: a workgroup consumes, at tile t, the slice it fetched at the previous
    tile for `t + nblk`.  With the walk of the large plan every tile's gradient rows are consumed exactly once; fetching for
    any other tile (t + 1, or t + nblk + 1) is noticed at these sizes, as is a fetch that does not stop at the job's rows."""
    rows, nblk = INPUT_SIZES[1][1], BWD_BIG_CAP
    ntiles = -(-rows // TR)

    def consumed(step, bounded=True):
        got = np.zeros(ntiles * TR, np.int64)
        wrong = 0
        for bid in range(nblk):
            held = bid
            for t in range(bid, ntiles, nblk):
                wrong += held != t
                lo, hi = held * TR, min(held * TR + TR, rows if bounded else ntiles * TR)
                if held < ntiles:
                    got[lo:hi] += 1
                held = t + step(nblk)
        return got, wrong
    got, wrong = consumed(lambda k: k)
    assert wrong == 0 and (got[:rows] == 1).all() and (got[rows:] == 0).all()
    assert consumed(lambda k: 1)[1] > 0 and consumed(lambda k: k + 1)[1] > 0
    assert consumed(lambda k: k, bounded=False)[0][rows:].sum() == TR - rows % TR        # rows past the job: outside its gradient


def test_stride_sizes():
    assert RBF_CAP_ROWS == 32768 and RBF_ROWS[5:] == [32768, 32769, 65541, 100003]
    blocks = lambda m: min(-(-m // RBF_ROW_SLOTS), RBF_BWD_BLOCKS)
    assert [blocks(m) for m in RBF_ROWS] == [0, 1, 1, 1, 2, 2048, 2048, 2048, 2048]
    passes = lambda m: -(-m // (blocks(m) * RBF_ROW_SLOTS)) if m else 0                 # edges of the busiest thread
    assert [passes(m) for m in RBF_ROWS] == [0, 1, 1, 1, 1, 1, 2, 3, 4]
    assert RBF_BWD_BLOCKS // RBF_FINAL_SLICES == 32
    # a partial loop without its stride (one edge per thread) leaves m - 32768 rows out: one row of 32 769 is already
    # 1 / sqrt(m) ~ 5e-3 of a sum of m random terms, against a bound of 1e-5
    assert ADAM_CAP == 4194304 and ADAM_N_PLAIN % 4 == 0 and ADAM_N_GROUPS % 64 == 0
    assert 3581100 < ADAM_CAP < min(ADAM_N_GROUPS, ADAM_N_PLAIN)                        # (3 581 100: the largest n elsewhere in the suite)
    for n in (ADAM_N_PLAIN, ADAM_N_GROUPS):
        n4 = n // 4
        assert min(-(-n4 // 256), ADAM_BLOCKS) == ADAM_BLOCKS and 0 < n4 - ADAM_BLOCKS * 256 < 256 * ADAM_BLOCKS   # a partial second pass
    assert (ADAM_N_PLAIN // 4 - ADAM_BLOCKS * 256) % 256 != 0                           # ... ending inside a workgroup
    for m in SBF_M:
        assert m in (1, SBF_ROWS - 1, SBF_ROWS, SBF_ROWS + 1) or (m > 64 * SBF_ROWS and m % SBF_ROWS not in (0, 1, SBF_ROWS - 1))
    assert 4099 % SBF_ROWS % SBF_ROW_STEP != 0                                          # ragged tile: threads stop at different rows


# ---- the GPU tests ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs an MI355X'
    from pamnet_amd import lib
    lib.load()
    return torch.device('cuda:0')


def _log(kernel, size, name, err, err32=None, bound=None):
    e32 = '        -' if err32 is None else '%9.3e' % err32
    bnd = '        -' if bound is None else '%9.3e' % bound
    print('TAIL %-26s %-22s %-10s err32=%s err=%9.3e bound=%s' % (kernel, size, name, e32, err, bnd))


def _poison(dev, floats):
    """The next torch.empty of this size most likely reuses this block: output the kernel does not write shows as NaN."""
    junk = torch.full((floats,), float('nan'), device=dev)
    del junk


# 1. pooling: every node exactly once
@pytest.mark.gpu
@pytest.mark.parametrize('sizes', [POOL_SIZES, [2200]], ids=['18-graphs', 'one-graph'])
def test_pool_counts_every_node_once(dev, sizes):
    from pamnet_amd import ops
    outs, atts, sign, twice = _pool_exact_inputs(sizes)
    g, batch, _ = _pool_graph(sizes, dev, False, None)
    B, n = len(sizes), int(sum(sizes))
    count = torch.tensor(sizes, dtype=torch.float64)
    for with_sign in (True, False):
        g.sign = sign.to(dev) if with_sign else None
        tw = twice * sign.long() if with_sign else twice
        want2 = torch.zeros(B, dtype=torch.int64).index_add_(0, batch, tw)              # twice the pooled sums, exact
        for mean in (False, True):
            _poison(dev, B)
            with torch.no_grad():
                out, node_out = ops.fuse_pool(outs.to(dev), atts.to(dev), g, mean)
            assert torch.equal(node_out.cpu(), tw.float() * 0.5)
            got = out.cpu()
            assert got.shape == (B,) and torch.isfinite(got).all()
            name = ('sign' if with_sign else 'nosign') + ('/mean' if mean else '/sum')
            if not mean:
                wrong = (got != want2.float() * 0.5).nonzero().view(-1).tolist()
                _log('pool exact', 'n=%d B=%d' % (n, B), name, float(len(wrong)), bound=0.0)
                assert not wrong, (name, [(sizes[b], float(got[b]), 0.5 * int(want2[b])) for b in wrong])
            else:
                ref = want2.double() * 0.5 / count.clamp(min=1)
                ulp = torch.from_numpy(np.spacing(ref.abs().float().numpy())).double()
                worst = float(((got.double() - ref).abs() / ulp).max())
                _log('pool exact', 'n=%d B=%d' % (n, B), name, worst, bound=1.0)
                assert ((got.double() - ref).abs() <= ulp).all(), name
                assert (got[count == 0] == 0).all()


# 2. fusion + pooling, the general case
PLANTS = [(0.0, 0.0), (0.0, 0.3), (-0.2, 0.0), (1e-30, -1e-30), (-1e-30, 1e-30), (0.7, 0.7), (-1.3, -1.3), (90.0, -90.0),
          (-90.0, 90.0)]


def _fuse_ref(outs, atts, sign, batch, B, mean, w, dtype):
    """O.fuse + O.segment_add in `dtype` on the CPU, from the fp32 inputs: (pooled, node_out, d outs, d atts)."""
    from oracle import pamnet_oracle as O
    L, n = outs.size(0) // 2, outs.size(1)
    o, a = outs.detach().clone().to(dtype).requires_grad_(), atts.detach().clone().to(dtype).requires_grad_()
    node = O.fuse([o[2 * l].view(1, n, 1) for l in range(L)], [o[2 * l + 1].view(1, n, 1) for l in range(L)],
                  [a[2 * l].view(1, n, 1) for l in range(L)], [a[2 * l + 1].view(1, n, 1) for l in range(L)])
    if sign is not None:
        node = node * sign.to(dtype).unsqueeze(-1)
    ref = O.segment_add(node, batch, B).view(-1)
    if mean:
        ref = ref / torch.bincount(batch, minlength=B).clamp(min=1)
    (ref * w.to(dtype)).sum().backward()
    return ref.detach(), node.detach().view(-1), o.grad, a.grad


@pytest.mark.gpu
@pytest.mark.parametrize('n_layer', [1, 3, 6])
def test_fuse_pool_general(dev, n_layer):
    from pamnet_amd import ops
    sizes = POOL_SIZES
    B, n = len(sizes), sum(sizes)
    gen = torch.Generator().manual_seed(50 + n_layer)
    g, batch, sign = _pool_graph(sizes, dev, True, gen)
    outs0 = torch.randn(2 * n_layer, n, generator=gen)
    atts0 = torch.randn(2 * n_layer, n, generator=gen)
    cols = torch.arange(5, n, 61)                                   # planted rows: in every graph of 65 nodes and more
    for k, v in enumerate(cols.tolist()):
        for l in range(n_layer):
            atts0[2 * l, v], atts0[2 * l + 1, v] = PLANTS[(k + l) % len(PLANTS)]
    assert len(cols) > 4 * len(PLANTS)
    w = torch.randn(B, generator=gen)
    count = torch.tensor(sizes, dtype=torch.float64)
    failures = []
    for with_sign in (True, False):
        g.sign = sign.to(dev) if with_sign else None
        for mean in (False, True):
            outs, atts = outs0.to(dev).requires_grad_(), atts0.to(dev).requires_grad_()
            _poison(dev, B)
            out, node_out = ops.fuse_pool(outs, atts, g, mean)
            (out * w.to(dev)).sum().backward()
            sg = sign if with_sign else None
            r64 = _fuse_ref(outs0, atts0, sg, batch, B, mean, w, torch.float64)
            r32 = _fuse_ref(outs0, atts0, sg, batch, B, mean, w, torch.float32)
            got = (out.detach().cpu(), node_out.cpu(), outs.grad.cpu(), atts.grad.cpu())
            name = 'L=%d %s/%s' % (n_layer, 'sign' if with_sign else 'nosign', 'mean' if mean else 'sum')
            for what, a, b32, b64 in zip(('out', 'node', 'douts', 'datts'), got, r32, r64):
                assert a.shape == b64.shape and torch.isfinite(a).all(), (name, what)
                err, err32 = maxnorm_err(a, b64), maxnorm_err(b32, b64)
                bound = max(5e-6, 2 * err32)
                _log('fuse_pool', 'n=%d B=%d' % (n, B), name + ' ' + what, err, err32, bound)
                if not err <= bound:
                    failures.append((name, what, err, bound))
            # per graph: against the graph's own sum of absolute terms
            mag = torch.zeros(B, dtype=torch.float64).index_add_(0, batch, r64[1].abs())
            if mean:
                mag = mag / count.clamp(min=1)
            live = mag > 0
            assert (got[0][~live] == 0).all() and int(live.sum()) == sum(s > 0 for s in sizes), name
            e = ((got[0].double() - r64[0]).abs()[live] / mag[live])
            e32 = ((r32[0].double() - r64[0]).abs()[live] / mag[live])
            bound = max(5e-6, 2 * float(e32.max()))
            _log('fuse_pool', 'n=%d B=%d' % (n, B), name + ' graph', float(e.max()), float(e32.max()), bound)
            if not float(e.max()) <= bound:
                failures.append((name, 'per graph', e.tolist(), bound))
    assert not failures, failures


# 3. zero nodes
@pytest.mark.gpu
@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
def test_fuse_pool_without_nodes_gives_zeros(dev, mean):
    from pamnet_amd import ops
    B = 3
    for with_sign in (True, False):
        g = types.SimpleNamespace(n_graphs=B, gptr=torch.zeros(B + 1, dtype=torch.int32, device=dev),
                                  node_graph=torch.zeros(0, dtype=torch.int32, device=dev),
                                  sign=torch.zeros(0, device=dev) if with_sign else None)
        outs = torch.zeros(2, 0, device=dev, requires_grad=True)
        atts = torch.zeros(2, 0, device=dev, requires_grad=True)
        _poison(dev, B)
        out, node_out = ops.fuse_pool(outs, atts, g, mean)
        assert out.shape == (B,) and node_out.shape == (0,)
        assert torch.equal(out.detach().cpu(), torch.zeros(B)), out                 # the reference's scatter into zeros
        (out * torch.randn(B, device=dev)).sum().backward()
        assert outs.grad.shape == (2, 0) and atts.grad.shape == (2, 0)


# 4. the Bessel-frequency gradient where threads stride
def _rbf_inputs(m, cutoff, dev):
    gen = torch.Generator().manual_seed(7 * m + 1)
    dist = (0.03 + 1.03 * torch.rand(m, generator=gen)) * cutoff                     # [0.03 c, 1.06 c]
    if m >= 15:
        dist[3], dist[m - 3] = 1.05 * cutoff, 1.02 * cutoff                         # beyond the cutoff: envelope 0
        dist[0], dist[m - 2] = 0.03 * cutoff, 0.999 * cutoff
        dist[m - 1] = 0.4 * cutoff                                                  # the last row (alone in its pass at cap + 1) counts
    freq = torch.arange(1, 17, dtype=torch.float32) * math.pi + 0.01 * torch.randn(16, generator=gen)
    w = torch.randn(m, 16, generator=gen)
    return dist.to(dev), freq.to(dev), w.to(dev)


@pytest.mark.parametrize('m', [m for m in RBF_ROWS if m > RBF_CAP_ROWS])
def test_rbf_rows_beyond_the_first_pass_matter(m):
    """What a partial kernel that does not stride would leave out (rows from 32 768 on) is far above the bound: at 32 769
    rows that is the last row alone."""
    from oracle import pamnet_oracle as O
    dist, freq, w = _rbf_inputs(m, 5.0, 'cpu')
    for p in (5, 4, 6):
        f = freq.double().requires_grad_()
        rows = O.bessel_rbf(dist.double(), f, 5.0, p) * w.double()
        whole, = torch.autograd.grad(rows.sum(), f, retain_graph=True)
        left_out, = torch.autograd.grad(rows[RBF_CAP_ROWS:].sum(), f)
        assert float(left_out.abs().max() / whole.abs().max()) > 1e-3, (m, p)


@pytest.mark.gpu
@pytest.mark.parametrize('m', RBF_ROWS)
@pytest.mark.parametrize('exponent', [5, 4, 6])                     # 5: pamnet_rbf_bwd_f32; 4, 6: pamnet_rbf_bwd_env_f32
def test_rbf_frequency_gradient(dev, m, exponent):
    from oracle import pamnet_oracle as O
    from pamnet_amd import ops
    cutoff = 5.0
    dist, freq0, w = _rbf_inputs(m, cutoff, dev)

    def hip():
        freq = freq0.clone().requires_grad_()
        _poison(dev, 16)
        (ops.rbf(dist, freq, cutoff, exponent=exponent) * w).sum().backward()
        return freq.grad
    got = hip()
    assert got.shape == (16,) and torch.isfinite(got).all()
    if m == 0:
        assert torch.equal(got.cpu(), torch.zeros(16))
        return
    if m >= 15:
        assert int((dist > cutoff).sum()) >= 2 and int((dist < cutoff).sum()) >= m // 2

    def ref(dtype):
        f = freq0.detach().clone().to(dtype).requires_grad_()
        (O.bessel_rbf(dist.to(dtype), f, cutoff, exponent) * w.to(dtype)).sum().backward()
        return f.grad.cpu()
    g64, g32 = ref(torch.float64), ref(torch.float32)
    err, err32 = maxnorm_err(got.cpu(), g64), maxnorm_err(g32, g64)
    bound = max(1e-5, 4 * err32)
    _log('rbf_bwd p=%d' % exponent, 'm=%d' % m, 'dfreq', err, err32, bound)
    assert err < bound, (m, exponent, err, err32)
    assert torch.equal(got, hip())                                  # fixed-order partials: the same bits again


# 5. the spherical-basis combine: gather and ragged tile
def _yl0(angle64, ns=7):
    """Y_l0(theta) = sqrt((2l + 1) / (4 pi)) P_l(cos theta), fp64 (numpy's Clenshaw evaluation of the Legendre series)."""
    ct = np.cos(angle64)
    return np.stack([math.sqrt((2 * l + 1) / (4 * math.pi)) * np.polynomial.legendre.legval(ct, [0.0] * l + [1.0])
                     for l in range(ns)], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize('m', SBF_M)
def test_sbf_combine_gathers_and_stops_at_the_last_row(dev, m):
    import models
    from oracle import pamnet_oracle as O
    from pamnet_amd import lib
    cutoff, SENT = 5.0, -7.5
    z32, norm = models.basis_tables(7, 6)
    zeros_d, norm_d = torch.from_numpy(z32).reshape(-1).to(dev), torch.from_numpy(norm).reshape(-1).to(dev)
    gen = torch.Generator().manual_seed(m)
    ang = torch.rand(m, generator=gen) * math.pi
    special = [0.0, math.pi / 2, math.pi]
    for k, r in enumerate(sorted({r for r in (0, 1, 2, m - 3, m - 2, m - 1) if 0 <= r < m})):
        ang[r] = special[k % 3]                                     # fp32 0, pi/2, pi: in the first tile and in the ragged one
    yl0 = _yl0(ang.double().numpy())
    assert np.abs(yl0 - O.sbf_angular(ang.double()).numpy()).max() < 1e-12          # the oracle's angular part, the same functions
    ang_d = ang.to(dev)
    for edges in SBF_EDGES:
        dist = (torch.linspace(0.03, 1.06, edges) if edges > 1 else torch.tensor([0.5])).to(dev) * cutoff
        idx = torch.randint(0, edges, (m,), generator=gen).to(torch.int32)
        if m >= 4099:
            assert len(set(idx.tolist())) == edges                  # every edge gathered, most of them many times
        st = lib.stream_of(dist)
        res = {}
        for form in ('fixed', 'table'):
            rad = torch.zeros(edges * 42, device=dev)
            sbf = torch.full(((m + SBF_ROWS) * 42,), SENT, device=dev)
            if form == 'fixed':
                lib.call('pamnet_sbf_radial_f32', lib.ptr(dist), cutoff, edges, lib.ptr(rad), st)
                lib.call('pamnet_sbf_combine_f32', lib.ptr(rad), lib.ptr(idx.to(dev)), lib.ptr(ang_d), m, lib.ptr(sbf), st)
            else:
                lib.call('pamnet_sbf_radial_tab_f32', lib.ptr(dist), cutoff, edges, 7, 6, 5, lib.ptr(zeros_d), lib.ptr(norm_d),
                         lib.ptr(rad), st)
                lib.call('pamnet_sbf_combine_tab_f32', lib.ptr(rad), lib.ptr(idx.to(dev)), lib.ptr(ang_d), m, 7, 6, lib.ptr(sbf), st)
            sbf = sbf.cpu().view(m + SBF_ROWS, 42)
            assert (sbf[m:] == SENT).all(), (form, m, edges)                          # nothing past the last row
            got = sbf[:m].double().numpy()
            assert np.isfinite(got).all() and not (got == SENT).any()
            rad64 = rad.cpu().double().view(edges, 42).numpy()                      # the kernel's own radial table
            ref = (rad64[idx.long().numpy()].reshape(m, 7, 6) * yl0.reshape(m, 7, 1)).reshape(m, 42)
            excess = np.abs(got - ref) - (2.0 ** -23 * np.abs(ref) + 1e-12)
            rel = float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30))[np.abs(ref) > 1e-6].max()) if (np.abs(ref) > 1e-6).any() else 0.0
            _log('sbf_combine ' + form, 'm=%d E=%d' % (m, edges), 'rel', rel, bound=2.0 ** -23)
            assert (excess <= 0).all(), (form, m, edges, float(excess.max()))
            assert np.abs(ref).max() > 0.1
            res[form] = sbf[:m]
        both = maxnorm_err(res['table'], res['fixed'])
        _log('sbf_combine both', 'm=%d E=%d' % (m, edges), 'maxnorm', both, bound=1e-6)
        assert both < 1e-6, (m, edges, both)


# 6. the input-stage backward in the large-launch plan
def _logged_ok(F, monkeypatch, kernel, size):
    real = F._ok

    def ok(a, b32, b64, floor=2e-6):
        res, (e, f) = real(a, b32, b64, floor)
        _log(kernel, size, tuple(a.shape).__repr__().replace(' ', ''), e, f, max(floor, 2 * f))
        return res, (e, f)
    monkeypatch.setattr(F, '_ok', ok)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['types_two', 'init18_two'])
@pytest.mark.parametrize('sizes', INPUT_SIZES, ids=['2048-tiles', '2049-tiles'])
def test_input_stage_around_the_plan_switch(dev, monkeypatch, sizes, variant):
    """test_hip_fused.test_input_stage itself (outputs at 2e-6, gradients at 1e-5 against torch fp32 and fp64, run-to-run
    identical bits, the one-layer entry point's bits) at the sizes whose plan test_input_stage_sizes_take_the_plans_they_are_meant_for
    proves."""
    import test_hip_fused as F
    _logged_ok(F, monkeypatch, 'input_stage ' + variant, 'e_g=%d' % sizes[1])
    F.test_input_stage(dev, sizes, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['rbf16', 'sbf42_kind'])           # rbf16: dx written, the prefetching body; sbf42_kind: the clamped loads
def test_embed_layer_alone_in_the_large_plan(dev, monkeypatch, case):
    import torch.nn as nn
    import test_hip_fused as F
    from pamnet_amd import fused
    rows = EMBED_ROWS
    _logged_ok(F, monkeypatch, 'embed ' + case, 'rows=%d' % rows)
    F.test_embed_layers(dev, rows, case)
    # run-to-run identical bits
    torch.manual_seed(rows)
    K, two = (16, False) if case == 'rbf16' else (42, True)
    lin0 = nn.Linear(K, F.D).to(dev)
    lin1 = nn.Linear(K, F.D).to(dev) if two else None
    x = torch.randn(rows, K, device=dev, requires_grad=not two)
    kind = (torch.rand(rows, device=dev) < 0.4).to(torch.int32) if two else None
    w = torch.randn(rows, F.D, device=dev)
    runs = []
    for _ in range(2):
        ps = list(lin0.parameters()) + (list(lin1.parameters()) if two else []) + [x]
        for p in ps:
            p.grad = None
        y = fused.embed(x, lin0, lin1, kind=kind, act=True)
        (y * w).sum().backward()
        runs.append([y.detach().clone()] + [p.grad.clone() for p in ps if p.grad is not None])
    assert len(runs[0]) == (4 if case == 'rbf16' else 5)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# 7. Adam + EMA past the grid cap
ADAM_TABLE = {'lr_scale': [1.0, 1.0, 10.0, 0.5], 'weight_decay': [1e-3, 5e-2, 1e-2, 0.0], 'frozen': [0, 1, 0, 0]}
CAP_CHUNK = ADAM_CAP // 64                                           # first 64-float chunk of the second pass
# a frozen run across the pass boundary, a one-chunk group and a group boundary inside the second pass
ADAM_SPANS = [(0, 1, 2), (1, CAP_CHUNK - 36, 0), (CAP_CHUNK - 36, CAP_CHUNK + 9, 1), (CAP_CHUNK + 9, CAP_CHUNK + 11, 0),
              (CAP_CHUNK + 11, CAP_CHUNK + 12, 3), (CAP_CHUNK + 12, CAP_CHUNK + 20, 0), (CAP_CHUNK + 20, CAP_CHUNK + 33, 2)]


def test_adam_spans():
    assert ADAM_SPANS[-1][1] * 64 == ADAM_N_GROUPS and ADAM_SPANS[0][0] == 0
    assert all(a[1] == b[0] for a, b in zip(ADAM_SPANS, ADAM_SPANS[1:]))
    lo, hi, grp = ADAM_SPANS[2]
    assert ADAM_TABLE['frozen'][grp] and lo < CAP_CHUNK < hi                          # frozen across the pass boundary
    assert sum(lo > CAP_CHUNK for lo, _, _ in ADAM_SPANS) >= 3                        # group boundaries inside the second pass


@pytest.mark.gpu
@pytest.mark.parametrize('entry,ema,zero_grad,decoupled', [('norm', True, 1, 0), ('norm', False, 0, 0), ('scalar', True, 0, 0),
                                                            ('scalar', False, 1, 0), ('groups', True, 0, 0), ('groups', False, 1, 1)])
def test_adam_ema_second_pass(dev, entry, ema, zero_grad, decoupled):
    """The three entry points at an n whose last 2052 (2112) floats are a second pass of the grid-stride loop, against
    _numpy_update of test_hip_trainer_groups.py at that file's RTOL = ATOL = 1e-6.

    The moments are a state Adam can reach.  With m = sum_k (1 - b1) b1^k g_k and v = sum_k (1 - b2) b2^k g_k^2,
    Cauchy-Schwarz gives m^2 <= v (1 - b1)^2 / ((1 - b2) (1 - b1^2 / b2)) = 52.9 v, so v is drawn as m^2 (0.02 + U[0, 1)) and
    an update stays O(lr).  The bound presumes that: the entry points take beta2 as a float, so the kernel's 1 - beta2 is
    1 - fl(0.999) = 0.99998713e-3, 1.3e-5 (relative) off the 1e-3 of torch's and _numpy_update's float64 scalar, which moves
    sqrt(v) by up to 6.5e-6 (relative) where v is far below (1 - b2) g^2.  Measured with v = 0.05 U[0, 1) beside m ~ 0.1 N(0, 1)
    at this n (the smallest v there are 0 and 3e-9: unreachable, single updates of 0.5): |p - ref| up to 2.1e-6, m, v and
    the shadow inside the bound; with reachable moments 2.4e-7 to 5.1e-7, the rounding of p itself."""
    from pamnet_amd import lib, ops
    from test_hip_trainer_groups import ATOL, RTOL, _numpy_update, _tables
    grouped = entry == 'groups'
    n = ADAM_N_GROUPS if grouped else ADAM_N_PLAIN
    torch.manual_seed(n + ema)
    P, G, M = torch.randn(n, device=dev), torch.randn(n, device=dev) * 0.3, torch.randn(n, device=dev) * 0.1
    V = M * M * (0.02 + torch.rand(n, device=dev))                   # a state Adam can reach (see the docstring)
    S = torch.randn(n, device=dev) if ema else None
    start = [t.cpu().numpy() for t in (P, G, M, V)] + [S.cpu().numpy() if ema else None]
    lr, b1, b2, eps, step, decay, max_norm = 2e-3, 0.9, 0.999, 1e-8, 3, 0.999, 5.0
    if grouped:
        table = ADAM_TABLE
        cmap = np.zeros(n // 64, np.uint8)
        for lo, hi, grp in ADAM_SPANS:
            cmap[lo:hi] = grp
        grp_of = np.repeat(cmap, 64)
    else:
        table = {'lr_scale': [1.0], 'weight_decay': [1e-3], 'frozen': [0]}
        grp_of = np.zeros(n, np.int64)
    want, norm64, clip = _numpy_update(*start, grp_of, table, lr, b1, b2, eps, step, decay, max_norm, bool(decoupled))
    assert clip < 1.0                                                # the clip binds
    st = lib.stream_of(P)
    nrm = torch.zeros(1, device=dev)
    if grouped:
        cm = torch.from_numpy(cmap).to(dev)
        sc, wd, fr = _tables(table)
        part = ops.sumsq_partials_masked(G, cm, 4, fr)
        lib.call('pamnet_adam_ema_groups_f32', lib.ptr(P), lib.ptr(G), lib.ptr(M), lib.ptr(V), lib.ptr(S), n, lib.ptr(cm), 4,
                 ctypes.addressof(sc), ctypes.addressof(wd), ctypes.addressof(fr), lr, b1, b2, eps, decoupled, step, decay,
                 lib.ptr(part), lib.ptr(nrm), max_norm, zero_grad, st)
    elif entry == 'norm':
        part = ops.sumsq_partials(G)
        lib.call('pamnet_adam_ema_norm_f32', lib.ptr(P), lib.ptr(G), lib.ptr(M), lib.ptr(V), lib.ptr(S), n, lr, b1, b2, eps,
                 table['weight_decay'][0], step, decay, lib.ptr(part), lib.ptr(nrm), max_norm, zero_grad, st)
    else:
        nrm = torch.tensor([norm64], dtype=torch.float32, device=dev)                # the device-scalar norm
        lib.call('pamnet_adam_ema_f32', lib.ptr(P), lib.ptr(G), lib.ptr(M), lib.ptr(V), lib.ptr(S), n, lr, b1, b2, eps,
                 table['weight_decay'][0], step, decay, lib.ptr(nrm), max_norm, zero_grad, st)
    torch.cuda.synchronize()
    assert abs(float(nrm) / norm64 - 1) <= RTOL
    g0 = torch.from_numpy(start[1])
    if zero_grad:
        assert float(G.abs().max()) == 0.0                           # everywhere, frozen chunks and the second pass included
    else:
        assert torch.equal(G.cpu(), g0)
    fz = torch.from_numpy(np.asarray(table['frozen'], bool)[grp_of])
    assert bool(fz[ADAM_CAP - 1]) == bool(fz[ADAM_CAP]) == grouped
    got = [P.cpu(), M.cpu(), V.cpu()] + ([S.cpu()] if ema else [])
    first = [start[0], start[2], start[3]] + ([start[4]] if ema else [])
    case = '%s ema=%d zg=%d' % (entry, ema, zero_grad)
    for name, a, wnt, a0 in zip(('p', 'm', 'v', 'shadow'), got, want, first):
        a0 = torch.from_numpy(a0)
        assert torch.equal(a[fz], a0[fz]), name                      # frozen: bitwise untouched
        live, ref = a[~fz].double(), torch.from_numpy(wnt)[~fz]
        excess = float(((live - ref).abs() - (ATOL + RTOL * ref.abs())).max())
        _log('adam ' + case, 'n=%d' % n, name, float((live - ref).abs().max()), bound=ATOL)
        assert excess <= 0, (name, excess)
        tail = slice(ADAM_CAP, n)                                    # the second pass, on its own
        moved = (a[tail] != a0[tail])
        assert bool(moved[~fz[tail]].float().mean() > 0.99), name
        assert torch.allclose(a[tail].double(), torch.from_numpy(wnt)[tail], rtol=RTOL, atol=ATOL), name
    if grouped:                                                      # both sides of every group boundary took their group's values
        for lo, hi, grp in ADAM_SPANS:
            for c in (lo, hi - 1):
                sl = slice(64 * c, 64 * c + 64)
                if table['frozen'][grp]:
                    assert torch.equal(got[0][sl], torch.from_numpy(start[0][sl])), c
                else:
                    assert torch.allclose(got[0][sl].double(), torch.from_numpy(want[0][sl]), rtol=RTOL, atol=ATOL), c
