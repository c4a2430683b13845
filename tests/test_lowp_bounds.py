"""CPU-only: the bounds the edge-case tests compute from the reference are
never looser than the thresholds of the older tests. Needs no GPU."""
import itertools

import _branch_oracle as bo
import _lowp_oracle as lo


def test_three_floor_within_existing_caps():
    """3 x floor <= cap for every tensor of every bf16/f16 case, the branch
    composites included, so tol = max(3 floor, 2 eps) is what is applied and
    the cap never bites. A case that is over gets a smaller depth (T or L),
    not a wider cap."""
    over = []
    n = 0
    for label, r in itertools.chain(lo.all_lowp_references(),
                                    bo.all_branch_references()):
        for name, fl in r.floor.items():
            n += 1
            if not 3.0 * fl <= r.cap[name]:
                over.append(f"{label} {name}: 3 x {fl:.4f} > {r.cap[name]}")
        assert 2.0 * lo.EPS[r.dtype] < lo.CAP_OUT
    assert n > 500          # the walk really covered the case lists
    assert not over, "\n".join(over)


def test_branch_draws_are_clear_of_the_relu_kinks():
    """The branch cases' draws keep every pre-activation of the two ReLUs
    whose gradient does not vanish at the kink further from zero than the
    roundings between a kernel and the oracle can move it (_branch_oracle).
    (That each recorded seed is the first to qualify is not asserted: the
    floors of the seeds before it depend on the CPU's low-precision kernels.)"""
    assert set(bo.BRANCH_SEEDS) == set(bo.BRANCH_CASES)
    for label, r in bo.all_branch_references():
        assert r.extra["relu_margin"] > bo.RELU_MARGIN, label


def test_branch_modules_on_cpu_equal_the_written_out_reference():
    """On the CPU the modules dispatch to the reference_impl functions, so
    CG_LSTM / GCN composed as the models compose them give exactly what
    reference_branch gives: output, dobs and every parameter gradient."""
    import copy
    for case in bo.BRANCH_CASES:
        r = bo.branch_reference(case, lo.BF16)
        rnn, gcn = (copy.deepcopy(m).double() for m in r.extra["modules"])
        got = bo.fwd_bwd(rnn, gcn, r.extra["csr"].dense_supports().double(),
                         r.inputs["obs"].double(), case[6], case[3] > 1)
        assert set(got) == set(r.want)
        for k in r.want:
            assert lo.relerr(got[k], r.want[k]) < 1e-12, (case, k)


def test_bound_rule():
    assert lo.bound(0.0, lo.BF16, 0.05) == 2.0 ** -7
    assert lo.bound(0.0, lo.F16, 0.05) == 2.0 ** -9
    assert lo.bound(0.01, lo.BF16, 0.05) == 0.03
    assert lo.bound(0.04, lo.F16, 0.1) == 0.1
