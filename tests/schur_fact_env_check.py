"""Child process of tests/test_gpu_schur_fact.py::test_eager_applications_count_alike: TP_GRAPH is read once per process.  Under
TP_GRAPH=0 (eager pc_apply, nothing recorded) every factorisation type applies K(A00) and K(S) as often as the recorded path
does and gives the oracle's result."""
from switches import child_main     # first: it puts the repository root on the path
import schur_fact_ref as SR
import test_gpu_schur_fact as T


def main():
    _, b, kw, opts = T.SYS["c4_2ph_cptr"]
    spec, u0, u, o, J, F = T.oracle(b, kw, opts)
    x = T.rand(u)
    h = T.engine(spec, u0, u, opts)
    h.vec_set("x", x)
    for fact in SR.FACTS:
        T.switch(h, schur_fact=fact)
        for _ in range(3):
            h.pc_apply("x", "y")
        i = h.schur_info()
        assert (i["k0_applies"], i["ks_applies"]) == ((6, 3) if fact == "full" else (3, 3)), (fact, i)
        assert T.rel2(h.vec_get("y"), SR.apply_fact(o.pc, "SI", x, fact)) < 1e-10, fact
    assert h.ksp_info()["pc_programs"] == 0
    h.close()


if __name__ == "__main__":
    child_main(main)
