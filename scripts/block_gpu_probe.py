"""Development probe: bjacobi BLOCK shapes on the GPU (tiles | boxes of several tiles | one block) -- Krylov iterations of the Newton
solve of the first timed step of a bench configuration (state after the untimed spin-up), ILU sweep time and launches per sweep
direction.  Usage: block_gpu_probe.py c4 [B0,B1,B2[:t0,t1,t2] | N | whole] ...   (N: bjacobi_blocks = N; 0 in a triple: whole extent)"""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench
from thermalporous_amd.engine import HipEngine

BIG = 1 << 30


def triple(s):
    return tuple(int(v) if int(v) > 0 else BIG for v in s.split(","))


def parse(a):
    if a == "whole":
        return dict(bjacobi_blocks=1)
    if "," not in a:
        return dict(bjacobi_blocks=int(a))
    blk, _, tile = a.partition(":")
    return dict(ilu_block=triple(blk), ilu_tile=triple(tile) if tile else None)


cfg = sys.argv[1]
m = bench.make_model(cfg)
m.start()
bench.spin_up(m, 200)
u = m.engine.get_state().copy()
dt = float(m.dt)
m.engine.close()
for arg in ["tiles"] + sys.argv[2:]:
    over = {} if arg == "tiles" else parse(arg)
    mm = bench.make_model(cfg, engine_factory=(lambda spec, opts: HipEngine(spec, dict(opts, **over))) if over else None)
    e = mm.engine
    for rep in range(2):
        e.set_state(u); e.set_old(u); e.set_dt(dt)
        t0 = time.perf_counter()
        r = e.newton_solve()
        wall = time.perf_counter() - t0
    e._ck(e.lib.tp_jacobian(e.ctx)); e.pc_setup()
    lay = e.ilu_layout()
    print(json.dumps(dict(arg=arg, block=list(lay["block"]), tile=[min(t, 9999) for t in e.opts["ilu_tile"]], nblocks=lay["nblocks"],
                          ntiles=lay["ntiles"], launches=lay["launches"], max_tiles_per_launch=lay["max_tiles_per_launch"],
                          nits=r["nits"], lits=r["lits"], reason=r["reason"], solve_ms=round(wall*1e3, 1),
                          ilu_solve_ms=round(e.time_kernel(1, 50), 4), pc_apply_ms=round(e.time_kernel(4, 20), 4),
                          ilu_factor_ms=round(e.time_kernel(6, 10), 4))), flush=True)
    e.close()
