"""bjacobi blocks larger than one tile (``sub_1_pc_bjacobi_blocks = N``, engine option ``ilu_block``) on the GPU against the
CPU oracle, which takes blocks of any size as its ``ilu_tile``.

A block is a box of whole cells cut into its own sweep tiles; couplings inside a block are kept, those across block faces
dropped; one launch sweeps block-local tile-diagonal d of every block.  Tolerances are the project's own:
ILU sweep and pc_apply 1e-10 in the 2-norm (1e-9 at full size), FGMRES counts +-1, Newton counts equal, state 1e-8."""
import ctypes as C
import threading

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

BIG = 1 << 30


def rel2(a, b):
    return np.linalg.norm((a - b).ravel())/max(np.linalg.norm(b.ravel()), 1e-300)


def expected_layout(n, block, tile):
    """The structure tp_ilu_layout must report, restated from the definition: per axis, blocks of `block` cells from the
    origin (ragged last), each cut into tiles of `tile` cells from ITS origin."""
    n = [int(v) for v in n]
    blk = [min(int(block[a]), n[a]) for a in range(3)]
    t = [min(int(tile[a]), blk[a]) for a in range(3)]
    per_axis = []                                   # block-local tile indices along each axis, block by block
    for a in range(3):
        loc = []
        for lo in range(0, n[a], blk[a]):
            ext = min(blk[a], n[a] - lo)
            loc.append(-(-ext//t[a]))
        per_axis.append(loc)
    nblocks = len(per_axis[0])*len(per_axis[1])*len(per_axis[2])
    ntiles = sum(per_axis[0])*sum(per_axis[1])*sum(per_axis[2])
    if all(max(p) == 1 for p in per_axis):          # every block is one tile: the per-tile path
        return dict(block=tuple(t), nblocks=ntiles, ntiles=ntiles, ndiag=1, max_tiles_per_launch=ntiles, launches=1)
    ndiag = max(per_axis[0]) + max(per_axis[1]) + max(per_axis[2]) - 2
    count = [0]*ndiag
    for c0 in per_axis[0]:
        for c1 in per_axis[1]:
            for c2 in per_axis[2]:
                for i in range(c0):
                    for j in range(c1):
                        for k in range(c2):
                            count[i + j + k] += 1
    return dict(block=tuple(blk), nblocks=nblocks, ntiles=ntiles, ndiag=ndiag, max_tiles_per_launch=max(count), launches=ndiag)


def setup_pair(spec, u0, oopts, hopts, seed=5, amp=0.3, dt=8640.0):
    from oracle.engine import OracleEngine
    from thermalporous_amd.engine import HipEngine
    o, h = OracleEngine(spec, oopts), HipEngine(spec, hopts)
    u = cases.perturbed_state(spec, seed=seed, amp=amp)
    for e in (o, h):
        e.set_old(u0)
        e.set_dt(dt)
        e.set_state(u)
    schur = oopts["pc"] in ("cptr", "fieldsplit_cd")
    out = o.jacobian(want_schur=schur)
    J, Sm = out if schur else (out, None)
    h.jacobian()
    o.pc.setup(J, Sm)
    h.pc_setup()
    return o, h, J


def check_stages(name, spec, u0, oopts, hopts, krylov=True):
    """ILU sweep, whole preconditioner and (krylov) FGMRES of the HIP engine with blocks against the oracle."""
    import oracle.linalg as la
    o, h, J = setup_pair(spec, u0, oopts, hopts)
    x = np.random.default_rng(11).standard_normal(J.shape[1:2] + J.shape[3:])
    h.vec_set("x", x)
    h.ilu_solve("x", "y")
    e_ilu = rel2(h.vec_get("y"), o.pc.ilu.solve(x))
    h.pc_apply("x", "y")
    e_pc = rel2(h.vec_get("y"), o.pc.apply(x))
    lay = h.ilu_layout()
    print("%s: layout %r  ilu %.2e  pc %.2e" % (name, lay, e_ilu, e_pc))
    assert e_ilu < 1e-10, (name, e_ilu)
    assert e_pc < 1e-10, (name, e_pc)
    if krylov:
        F = o.residual()
        h.residual()
        h.copy_residual_to("b")
        its_h, reason_h, _ = h.fgmres("b", "d")
        d_o, its_o, reason_o, _ = la.fgmres(lambda v: la.spmv_block(J, v), o.pc.apply, F, rtol=o.opts["ksp_rtol"],
                                            maxit=o.opts["ksp_max_it"], restart=o.opts["ksp_restart"])
        print("%s: fgmres %d (oracle %d)" % (name, its_h, its_o))
        assert reason_h == reason_o == 2 and abs(its_h - its_o) <= 1, (name, its_h, its_o)
        assert rel2(h.vec_get("d"), d_o) < 1e-6
    opts = dict(h.opts)
    h.close()
    return lay, opts


# ---- counts that no tiling of one-wavefront tiles gives ---------------------------------------------------------------------
COUNTS = [
    ("c4_2ph_cptr_2blocks", cases.c4_spe10_3d, dict(Nx=11, Ny=13, Nz=17, nphase=2), dict(pc="cptr", bjacobi_blocks=2), (17, 11, 7)),
    ("c3_1ph_cpr_2blocks", cases.c3_spe10_2d, dict(Nx=30, Ny=140, nphase=1), dict(pc="cpr", bjacobi_blocks=2), (30, 70, 1)),
    ("c4_1ph_cprQI_4blocks", cases.c4_spe10_3d, dict(Nx=16, Ny=18, Nz=9, nphase=1), dict(pc="cpr", decoup="QI", bjacobi_blocks=4), (9, 8, 9)),
]


@pytest.mark.parametrize("name,builder,kw,opts,block", COUNTS, ids=[c[0] for c in COUNTS])
def test_block_counts_beyond_one_wavefront(name, builder, kw, opts, block):
    from oracle.engine import blocks_to_tile
    from thermalporous_amd.engine import tiles_for_blocks
    spec, u0, *_ = builder(**kw)
    with pytest.raises(NotImplementedError):
        tiles_for_blocks(spec["n"], opts["bjacobi_blocks"])
    want = tuple(blocks_to_tile(spec["n"], opts["bjacobi_blocks"]))
    if block is not None:
        assert want == block
    lay, hopts = check_stages(name, spec, u0, opts, opts)
    assert tuple(hopts["ilu_block"]) == want and not hopts["ilu_whole"]
    assert lay == expected_layout(spec["n"], want, hopts["ilu_tile"])
    assert lay["block"] == want and lay["nblocks"] == opts["bjacobi_blocks"] and lay["ndiag"] > 1


# ---- explicit boxes: ragged last block, partial tiles on every axis, cuts along axis 0 --------------------------------------
EXPLICIT = [
    ("ragged_3d_2x2x2", dict(Nx=11, Ny=13, Nz=17, nphase=2), dict(pc="cptr"), (9, 6, 7), (5, 4, 3)),
    ("blocks_2x2_1ph", dict(Nx=11, Ny=13, Nz=17, nphase=1), dict(pc="cpr", decoup="TI"), (BIG, 6, 7), (6, 4, 3)),
    ("blocks_3x3", dict(Nx=11, Ny=13, Nz=17, nphase=2), dict(pc="cpr", decoup="QI"), (BIG, 4, 5), (5, 3, 2)),
    ("cptr_a11", dict(Nx=7, Ny=8, Nz=6, nphase=2), dict(pc="cptr", schur_a11=True), (4, 4, 5), (3, 3, 2)),
    ("axis0_cuts_only", dict(Nx=5, Ny=6, Nz=19, nphase=2), dict(pc="cptr"), (7, BIG, BIG), (3, 5, 6)),
    ("one_cell_tiles", dict(Nx=4, Ny=5, Nz=6, nphase=2), dict(pc="cptr"), (4, 3, 3), (1, 1, 1)),
    ("whole_as_block", dict(Nx=7, Ny=13, Nz=9, nphase=2), dict(pc="cptr"), (BIG, BIG, BIG), (4, 3, 4)),
]


@pytest.mark.parametrize("name,kw,opts,block,tile", EXPLICIT, ids=[c[0] for c in EXPLICIT])
def test_explicit_blocks(name, kw, opts, block, tile):
    spec, u0, *_ = cases.c4_spe10_3d(**kw)
    lay, _ = check_stages(name, spec, u0, dict(opts, ilu_tile=block), dict(opts, ilu_block=block, ilu_tile=tile))
    assert lay == expected_layout(spec["n"], block, tile)
    assert lay["launches"] == lay["ndiag"] > 1


def test_layout_of_the_worked_example():
    """17 x 11 x 13 cells, blocks 9 x 6 x 7, tiles 5 x 4 x 3: 2 x 2 x 2 blocks.  Axis 0: blocks of 9 and 8 cells, 2 tiles each;
    axis 1: 6 and 5 cells, 2 tiles each; axis 2: 7 and 6 cells, 3 and 2 tiles -- 4 x 4 x 5 = 80 tiles.  Four blocks hold 2 x 2 x 3
    tiles (diagonals of 1, 3, 4, 3, 1 tiles), four hold 2 x 2 x 2 (1, 3, 3, 1): 5 launches, the fullest of 4*4 + 4*3 = 28 tiles."""
    from thermalporous_amd.engine import HipEngine
    spec, u0, *_ = cases.c4_spe10_3d(Nx=11, Ny=13, Nz=17, nphase=2)
    assert tuple(spec["n"]) == (17, 11, 13)
    h = HipEngine(spec, dict(pc="cptr", ilu_block=(9, 6, 7), ilu_tile=(5, 4, 3)))
    lay = h.ilu_layout()
    assert lay == dict(block=(9, 6, 7), nblocks=8, ntiles=4*4*5, ndiag=5, max_tiles_per_launch=28, launches=5)
    assert lay == expected_layout(spec["n"], (9, 6, 7), (5, 4, 3))
    # the default: every tile is a block, one launch
    h.set_options(ilu_block=None)
    t = h.opts["ilu_tile"]
    lay = h.ilu_layout()
    assert lay["ndiag"] == 1 and lay["launches"] == 1 and lay["nblocks"] == lay["ntiles"] == lay["max_tiles_per_launch"]
    assert lay["block"] == (min(t[0], 17), min(t[1], 11), min(t[2], 13))
    # one block per rank
    h.set_options(ilu_whole=True)
    lay = h.ilu_layout()
    assert lay["block"] == (17, 11, 13) and lay["nblocks"] == 1 and lay["ndiag"] == lay["launches"] == 4 + 3 + 5 - 2
    h.close()


def test_block_equal_to_tile_is_the_tile_path_bit_for_bit():
    """Blocks that hold one tile each are today's tiles: same kernels, same launch, same bits (default 3-D and 2-D tiles and an
    explicit tile); a block SMALLER than the tile clips the tile."""
    from thermalporous_amd.engine import HipEngine
    for builder, kw, opts in ((cases.c4_spe10_3d, dict(Nx=11, Ny=13, Nz=17, nphase=2), dict(pc="cptr")),
                              (cases.c3_spe10_2d, dict(Nx=30, Ny=70, nphase=2), dict(pc="cptr")),
                              (cases.c4_spe10_3d, dict(Nx=11, Ny=13, Nz=17, nphase=1), dict(pc="cpr", ilu_tile=(5, 4, 7)))):
        spec, u0, *_ = builder(**kw)
        u = cases.perturbed_state(spec, seed=5, amp=0.3)
        x = np.random.default_rng(11).standard_normal(u.shape)
        res = []
        tile = None
        for variant in ("tiles", "block=tile", "block<tile"):
            o = dict(opts)
            if variant == "block=tile":
                o.update(ilu_tile=tile, ilu_block=tile)
            elif variant == "block<tile":
                o.update(ilu_tile=(BIG, tile[1], 64//tile[1]), ilu_block=tile)      # (64//t1 >= t2)
            h = HipEngine(spec, o)
            tile = tuple(h.opts["ilu_tile"]) if tile is None else tile
            h.set_old(u0)
            h.set_dt(8640.0)
            h.set_state(u)
            h.jacobian()
            h.pc_setup()
            h.vec_set("x", x)
            h.ilu_solve("x", "y")
            res.append((h.vec_get("y").copy(), h.ilu_layout()))
            h.close()
        assert res[0][1]["ndiag"] == 1 and res[0][1]["launches"] == 1
        for y, lay in res[1:]:
            assert lay == res[0][1]
            assert np.array_equal(y, res[0][0])


def test_ilu1_refuses_multi_tile_blocks():
    from thermalporous_amd.engine import HipEngine, EngineError
    spec, u0, *_ = cases.c4_spe10_3d(Nx=7, Ny=8, Nz=6, nphase=2)
    h = HipEngine(spec, dict(pc="cpr", ilu_levels=1, ilu_block=(4, 4, 5), ilu_tile=(3, 3, 2)))
    with pytest.raises(EngineError, match="ILU\\(0\\)"):
        h.ilu_layout()
    h.close()


def test_seeded_fuzz_over_boxes_blocks_and_tiles():
    """20 seeded draws of (box, phases, preconditioner, block, tile), every one valid (t1*t2 <= 64, block >= 1 cell per
    axis) and every one checked: the structure against its definition, sweep and preconditioner against the oracle."""
    rng = np.random.default_rng(20251016)
    pcs = [dict(pc="cptr"), dict(pc="cpr", decoup="QI"), dict(pc="cpr"), dict(pc="cptr", schur_a11=True)]
    multi = 0
    for draw in range(20):
        nph = int(rng.integers(1, 3))
        if draw % 5 == 4:                          # a 2-D box
            spec, u0, *_ = cases.c3_spe10_2d(Nx=int(rng.integers(3, 24)), Ny=int(rng.integers(3, 40)), nphase=nph)
        else:
            spec, u0, *_ = cases.c4_spe10_3d(Nx=int(rng.integers(2, 13)), Ny=int(rng.integers(2, 15)), Nz=int(rng.integers(2, 16)),
                                             nphase=nph)
        n = [int(v) for v in spec["n"]]
        opts = dict(pcs[int(rng.integers(0, len(pcs)))])
        if nph == 1:
            opts = dict(pc="cpr", decoup=opts.get("decoup", "No"))
        block = tuple(int(rng.integers(1, n[a] + 1)) if rng.random() < 0.8 else BIG for a in range(3))
        while True:
            tile = tuple(int(rng.integers(1, min(n[a], 9) + 1)) for a in range(3))
            if tile[1]*tile[2] <= 64:
                break
        if rng.random() < 0.3:
            tile = (BIG,) + tile[1:]
        name = "draw%02d n=%r block=%r tile=%r %r" % (draw, n, [min(b, 9999) for b in block], [min(t, 9999) for t in tile], opts)
        lay, _ = check_stages(name, spec, u0, dict(opts, ilu_tile=block), dict(opts, ilu_block=block, ilu_tile=tile), krylov=False)
        assert lay == expected_layout(n, block, tile), name
        multi += lay["ndiag"] > 1
    assert multi >= 10          # (most draws have blocks of several tiles)


def test_newton_solve_on_blocks():
    from oracle.engine import OracleEngine
    from thermalporous_amd.engine import HipEngine
    spec, u0, *_ = cases.c4_spe10_3d(Nx=11, Ny=13, Nz=17, nphase=2)
    opts = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25, bjacobi_blocks=2)
    o, h = OracleEngine(spec, opts), HipEngine(spec, opts)
    assert h.opts["ilu_block"] == (17, 11, 7)
    for e in (o, h):
        e.set_state(u0)
    for step in range(2):
        for e in (o, h):
            e.set_old(e.get_state() if e is o else None)
            e.set_dt(86.4)
        ro, rh = o.newton_solve(), h.newton_solve()
        print("newton step %d: hip %r oracle %r" % (step, rh, ro))
        assert ro["reason"] > 0 and rh["reason"] == ro["reason"], (ro, rh)
        assert rh["nits"] == ro["nits"]
        assert abs(rh["lits"] - ro["lits"]) <= ro["nits"]          # +-1 per linear solve
        uo, uh = o.get_state(), h.get_state()
        assert rel2(uh[0], uo[0]) < 1e-8 and rel2(uh[1], uo[1]) < 1e-8
        assert np.abs(uh[2] - uo[2]).max() < 1e-8
    h.close()


def test_time_loop_with_the_dictionary_spelling():
    """``sub_1_pc_bjacobi_blocks: 2`` in a reference-style parameter dictionary (pc_cptr, twophase.py:531-550, plus the key of
    tests/test_homo_wells.py:112) through TwoPhase.solve().  The grid is 9 x 13 x 17 cells: every cut into two boxes leaves more
    than 64 columns per box, so no tiling of one-wavefront tiles gives this count."""
    from oracle.engine import OracleEngine
    from thermalporous_amd.engine import tiles_for_blocks
    from thermalporous_amd.twophase import TwoPhase
    v_cycle = {"ksp_type": "preonly", "pc_type": "hypre", "pc_hypre_type": "boomeramg", "pc_hypre_boomeramg_max_iter": 1}
    d = {"snes_type": "newtonls", "snes_max_it": 25, "ksp_type": "fgmres", "ksp_max_it": 200, "ksp_gmres_restart": 200,
         "ksp_rtol": 1e-8, "pc_type": "composite", "pc_composite_type": "multiplicative", "pc_composite_pcs": "python,bjacobi",
         "sub_0_pc_python_type": "thermalporous.preconditioners.CPTRStage1PC", "sub_0_cpr_stage1_pc_type": "fieldsplit",
         "sub_0_cpr_stage1_pc_fieldsplit_type": "schur", "sub_0_cpr_stage1_pc_fieldsplit_schur_fact_type": "FULL",
         "sub_0_cpr_stage1_fieldsplit_1_ksp_type": "preonly", "sub_0_cpr_stage1_fieldsplit_1_pc_type": "python",
         "sub_0_cpr_stage1_fieldsplit_1_pc_python_type": "thermalporous.preconditioners.ConvDiffSchurTwoPhasesPC",
         "sub_0_cpr_stage1_fieldsplit_1_schur": v_cycle, "sub_0_cpr_stage1_fieldsplit_0": v_cycle,
         "sub_1_pc_bjacobi_blocks": 2, "sub_1_sub_pc_type": "ilu", "sub_1_sub_pc_factor_levels": 0, "mat_type": "aij"}
    res = []
    for factory in (OracleEngine, None):
        spec, u0, p, g, c = cases.c4_spe10_3d(Nx=13, Ny=17, Nz=9, nphase=2)
        with pytest.raises(NotImplementedError):
            tiles_for_blocks(spec["n"], 2)
        m = TwoPhase(g, c, p, end=0.02, maxdt=0.01, small_dt_start=False, solver_parameters=d,
                     filename=None, verbosity=False, _engine_factory=factory)
        assert m.engine_opts["bjacobi_blocks"] == 2 and m.engine_opts["pc"] == "cptr"
        m.solve()
        if factory is None:
            assert m.engine.opts["ilu_block"] is not None and not m.engine.opts["ilu_whole"]
            lay = m.engine.ilu_layout()
            assert lay["nblocks"] == 2 and lay["ndiag"] > 1
        assert m.failed_solves == 0
        res.append((m.nits_vec, m.lits_vec, [x.copy() for x in m.u.dat.data_ro]))
    assert res[0][0] == res[1][0] and len(res[0][0]) >= 2
    assert all(abs(a - b) <= 1 for a, b in zip(res[0][1], res[1][1]))
    for a, b in zip(res[1][2], res[0][2]):
        assert rel2(a, b) < 1e-7


def _ilu_on_slabs(spec, opts, u0, u, dt, xs, nranks):
    """tp_ilu0_solve of the global vector xs on an in-process group of `nranks` slabs; the assembled global result."""
    from thermalporous_amd import engine as E
    lib = E.load_library()
    group = C.c_void_p()
    assert lib.tp_local_group_create(nranks, C.byref(group)) == 0
    out, err = [None]*nranks, []

    def worker(rank):
        try:
            h = E.HipEngine(spec, opts, rank=rank, nranks=nranks, local_group=group)
            h.set_old(u0)
            h.set_dt(dt)
            h.set_state(u)
            h.jacobian()
            h.pc_setup()
            h.vec_set("x", xs)
            h.ilu_solve("x", "y")
            out[rank] = (h.vec_get("y"), h.amg_layout(0)[0], h.ilu_layout())
            h.close()
        except Exception as e:      # noqa: BLE001
            err.append((rank, repr(e)))
    ts = [threading.Thread(target=worker, args=(r,)) for r in range(nranks)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts), "slab worker hung"
    lib.tp_local_group_destroy(group)
    assert not err, err
    assert all(o[1] == 0 for o in out)                    # replicated hierarchy
    assert all(o[2]["nblocks"] == 1 for o in out)         # one block per slab
    return np.concatenate([o[0] for o in out], axis=-3)


@pytest.mark.parametrize("nranks", [2, 3])
def test_blocks_as_slabs_state_the_n_slab_operator(nranks):
    """ONE context whose blocks are the slabs, ilu_block = (n0, n1, n2/N), applies the stage-2 operator of an N-slab run with one
    block per rank (PETSc's default bjacobi under mpiexec -n N) without any of the slab group's halo, exchange or per-rank code:
    both equal one another and the oracle with nslabs = N.  (The ILU stage is compared: the AMG layouts are not shown to
    coincide.)"""
    from oracle.engine import OracleEngine
    from thermalporous_amd.engine import HipEngine
    spec, u0, *_ = cases.c4_spe10_3d(Nx=9, Ny=12, Nz=8, nphase=2)
    n = tuple(int(v) for v in spec["n"])
    assert n[2] % nranks == 0
    u = cases.perturbed_state(spec, seed=5, amp=0.2)
    xs = np.random.default_rng(11).standard_normal(u.shape)
    base = dict(pc="cptr", amg_gather_cells=-1, ilu_tile=(4, 3, 3))
    many = _ilu_on_slabs(spec, dict(base, ilu_whole=True), u0, u, 3000.0, xs, nranks)
    h = HipEngine(spec, dict(base, ilu_block=(n[0], n[1], n[2]//nranks)))
    h.set_old(u0)
    h.set_dt(3000.0)
    h.set_state(u)
    h.jacobian()
    h.pc_setup()
    h.vec_set("x", xs)
    h.ilu_solve("x", "y")
    one = h.vec_get("y")
    lay = h.ilu_layout()
    h.close()
    assert lay["nblocks"] == nranks and lay["block"] == (n[0], n[1], n[2]//nranks)
    o = OracleEngine(spec, dict(pc="cptr", ilu_whole=True, nslabs=nranks))
    o.set_old(u0)
    o.set_dt(3000.0)
    o.set_state(u)
    J, Sm = o.jacobian(want_schur=True)
    o.pc.setup(J, Sm)
    ref = o.pc.ilu.solve(xs)
    e1, e2, e3 = rel2(one, many), rel2(one, ref), rel2(many, ref)
    print("blocks as %d slabs: one-context vs group %.2e, vs oracle %.2e; group vs oracle %.2e" % (nranks, e1, e2, e3))
    assert e1 < 1e-10 and e2 < 1e-10 and e3 < 1e-10


def test_c4_true_size_eight_blocks_vs_cport():
    """``sub_1_pc_bjacobi_blocks: 8`` at BASELINE config 4's size (60x220x85 cells): eight boxes of 85 x 30 x 55 cells, each swept
    tile-diagonal by tile-diagonal -- sweep, whole preconditioner and FGMRES against oracle/cport (mirrors
    test_whole_slab_ilu0_true_sizes_c2_c4)."""
    from oracle.cport import CPortEngine
    from thermalporous_amd.engine import HipEngine
    spec, u0, *_ = cases.c4_spe10_3d(60, 220, 85)
    u = cases.perturbed_state(spec, seed=1, amp=0.05)
    x = np.random.default_rng(11).standard_normal(u.shape)
    opts = dict(pc="cptr", ksp_rtol=1e-8, snes_max_it=25, bjacobi_blocks=8)
    c, h = CPortEngine(spec, opts), HipEngine(spec, opts)
    assert tuple(c.opts["ilu_tile"]) == (85, 30, 55) == tuple(h.opts["ilu_block"])
    for e in (c, h):
        e.set_old(u0)
        e.set_dt(600.0)
        e.set_state(u)
    c.residual()
    c.jacobian()
    h.jacobian()
    c.pc_setup()
    h.pc_setup()
    assert c.ntiles() == 8
    lay = h.ilu_layout()
    assert lay == expected_layout(spec["n"], (85, 30, 55), h.opts["ilu_tile"]) and lay["nblocks"] == 8
    h.vec_set("x", x)
    h.ilu_solve("x", "y")
    e_ilu = rel2(h.vec_get("y"), c.ilu_solve(x))
    h.pc_apply("x", "y")
    e_pc = rel2(h.vec_get("y"), c.pc_apply(x))
    print("C4, 8 blocks: layout %r  sweep %.2e  pc %.2e" % (lay, e_ilu, e_pc))
    assert e_ilu < 1e-10
    assert e_pc < 1e-9
    F = c.residual()
    h.residual()
    h.copy_residual_to("b")
    its_h, reason_h, _ = h.fgmres("b", "d")
    d_c, its_c, reason_c, _ = c.fgmres(F)
    print("C4, 8 blocks: FGMRES %d (cport %d), sweep %.3f ms" % (its_h, its_c, h.time_kernel(1, 10)))
    assert reason_h == reason_c == 2 and abs(its_h - its_c) <= 1, (its_h, its_c)
    assert rel2(h.vec_get("d"), d_c) < 1e-6
    h.close()
