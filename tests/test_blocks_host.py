"""Host logic of bjacobi blocks larger than one tile (``sub_1_pc_bjacobi_blocks = N``, engine option ``ilu_block``): the
block rule equals the oracle's, every branch of the engine's option resolution, and the option passes the preset parser.
Nothing here loads the HIP library."""
import pytest

from thermalporous_amd import engine as E
from thermalporous_amd.solver_options import engine_options

BIG = 1 << 30

GRIDS = [
    ((85, 60, 220), 1), ((85, 60, 220), 8), ((85, 60, 220), 16), ((85, 60, 220), 224), ((400, 400, 1), 4),
    ((400, 400, 1), 1), ((400, 400, 1), 16), ((17, 11, 13), 2), ((17, 11, 13), 4), ((17, 11, 13), 6), ((30, 140, 1), 2),
    ((60, 220, 1), 3), ((9, 7, 13), 2), ((9, 7, 13), 13), ((5, 1, 1), 5), ((12, 12, 12), 27), ((60, 8, 8), 1),
]


@pytest.mark.parametrize("n,nb", GRIDS)
def test_blocks_for_count_is_the_oracle_rule(n, nb):
    from oracle.engine import blocks_to_tile
    blk = E.blocks_for_count(n, nb)
    assert tuple(blk) == tuple(blocks_to_tile(n, nb))
    cut = [-(-n[a]//blk[a]) for a in range(3)]
    assert cut[0]*cut[1]*cut[2] == nb


def test_blocks_for_count_refuses_what_no_box_tiling_gives():
    with pytest.raises(NotImplementedError):
        E.blocks_for_count((4, 4, 1), 7)
    with pytest.raises(ValueError):
        E.blocks_for_count((4, 4, 1), 0)


def _opts(**kw):
    return dict(E.DEFAULT_OPTS, **kw)


def test_count_one_and_count_nranks_stay_whole_slab():
    for nranks, nb in ((1, 1), (3, 3)):
        o = E.resolve_ilu_options(_opts(bjacobi_blocks=nb), (85, 60, 220), nranks)
        assert o["ilu_whole"] is True and o["ilu_block"] is None
        assert o["ilu_tile"] == E.whole_ilu_tile((85, 60, 220), nslabs=nranks)


def test_count_that_fits_tiles_keeps_the_tile_path():
    o = E.resolve_ilu_options(_opts(bjacobi_blocks=224), (85, 60, 220))
    assert o["ilu_tile"] == (85, 9, 7) and o["ilu_block"] is None and not o["ilu_whole"]
    o = E.resolve_ilu_options(_opts(bjacobi_blocks=16), (400, 400, 1))
    assert o["ilu_tile"] == (400, 25, 1) and o["ilu_block"] is None


@pytest.mark.parametrize("n,nb,block", [((85, 60, 220), 8, (85, 30, 55)), ((400, 400, 1), 4, (400, 100, 1)),
                                        ((17, 11, 13), 2, (17, 11, 7)), ((30, 140, 1), 2, (30, 70, 1))])
def test_count_beyond_one_wavefront_becomes_boxes_of_tiles(n, nb, block):
    with pytest.raises(NotImplementedError):
        E.tiles_for_blocks(n, nb)
    o = E.resolve_ilu_options(_opts(bjacobi_blocks=nb, ilu_tile=(3, 3, 3)), n)      # (the count overrides ilu_tile)
    assert o["ilu_block"] == block and not o["ilu_whole"]
    t = o["ilu_tile"]
    assert t == E.block_ilu_tile(block) == E.whole_ilu_tile(block)
    assert min(t[1], block[1])*min(t[2], block[2]) <= 64
    assert any(min(t[a], block[a]) < block[a] for a in range(3))                    # several tiles per block


def test_no_box_tiling_still_raises():
    with pytest.raises(NotImplementedError):
        E.resolve_ilu_options(_opts(bjacobi_blocks=7), (4, 4, 1))


def test_explicit_block_and_slabs():
    o = E.resolve_ilu_options(_opts(ilu_block=(9, 6, 7), ilu_tile=(5, 4, 3)), (17, 11, 13))
    assert o["ilu_block"] == (9, 6, 7) and o["ilu_tile"] == (5, 4, 3) and not o["ilu_whole"]
    # no tile given: the whole-slab rule on the block, clipped to the slab
    o = E.resolve_ilu_options(_opts(ilu_block=(BIG, BIG, 4)), (17, 11, 12), nranks=3)
    assert o["ilu_block"] == (BIG, BIG, 4) and o["ilu_tile"] == E.whole_ilu_tile((17, 11, 4))
    # several slabs: an explicit block is accepted, a count other than the slab count is not
    with pytest.raises(E.EngineError):
        E.resolve_ilu_options(_opts(bjacobi_blocks=4), (17, 11, 12), nranks=2)
    with pytest.raises(E.EngineError):
        E.resolve_ilu_options(_opts(ilu_block=(9, 6, 7), ilu_whole=True), (17, 11, 13))
    with pytest.raises(ValueError):
        E.resolve_ilu_options(_opts(ilu_block=(9, 0, 7)), (17, 11, 13))


def test_defaults_are_untouched():
    o = E.resolve_ilu_options(_opts(), (85, 60, 220))
    assert o["ilu_tile"] == E.default_ilu_tile((85, 60, 220)) and o["ilu_block"] is None and not o["ilu_whole"]
    opt = E.HipEngine._make_options(o)
    assert list(opt.ilu_block) == [0, 0, 0]
    o = E.resolve_ilu_options(_opts(ilu_block=(BIG, 30, 55)), (85, 60, 220))
    assert list(E.HipEngine._make_options(o).ilu_block) == [BIG, 30, 55]


def test_engine_options_accepts_ilu_block_and_both_spellings_of_the_count():
    d = {"snes_type": "newtonls", "ksp_type": "fgmres", "pc_type": "composite", "pc_composite_type": "multiplicative",
         "pc_composite_pcs": "python,bjacobi", "sub_0_pc_python_type": "thermalporous.preconditioners.CPRStage1PC",
         "sub_0_cpr_stage1": {"ksp_type": "preonly", "pc_type": "hypre", "pc_hypre_type": "boomeramg",
                              "pc_hypre_boomeramg_max_iter": 1},
         "sub_1_sub_pc_type": "ilu", "sub_1_sub_pc_factor_levels": 0, "mat_type": "aij"}
    o = engine_options({**d, "ilu_block": (9, 6, 7), "ilu_tile": (5, 4, 3)}, "Single phase")
    assert o["ilu_block"] == (9, 6, 7) and o["ilu_tile"] == (5, 4, 3)
    assert engine_options({**d, "sub_1_pc_bjacobi_blocks": 8}, "Single phase")["bjacobi_blocks"] == 8
    assert engine_options({**d, "sub_1": {"pc_bjacobi_blocks": 8}}, "Single phase")["bjacobi_blocks"] == 8
    assert engine_options(d, "Single phase")["ilu_block"] is None
