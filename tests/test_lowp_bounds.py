"""CPU-only: the bounds the edge-case tests compute from the reference are
never looser than the thresholds of the older tests. Needs no GPU."""
import _lowp_oracle as lo


def test_three_floor_within_existing_caps():
    """3 x floor <= cap for every tensor of every bf16/f16 case, so
    tol = max(3 floor, 2 eps) is what is applied and the cap never bites.
    A case that is over gets a smaller depth (T or L), not a wider cap."""
    over = []
    n = 0
    for label, r in lo.all_lowp_references():
        for name, fl in r.floor.items():
            n += 1
            if not 3.0 * fl <= r.cap[name]:
                over.append(f"{label} {name}: 3 x {fl:.4f} > {r.cap[name]}")
        assert 2.0 * lo.EPS[r.dtype] < lo.CAP_OUT
    assert n > 500          # the walk really covered the case lists
    assert not over, "\n".join(over)


def test_bound_rule():
    assert lo.bound(0.0, lo.BF16, 0.05) == 2.0 ** -7
    assert lo.bound(0.0, lo.F16, 0.05) == 2.0 ** -9
    assert lo.bound(0.01, lo.BF16, 0.05) == 0.03
    assert lo.bound(0.04, lo.F16, 0.1) == 0.1
