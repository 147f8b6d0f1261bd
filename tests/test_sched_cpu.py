"""CPU tier: the hazard analysis behind the lane scheduler and the chain pass, on hand-written accesses (no plan, no library)."""
from unet_zoo_amd import _sched


def test_hazard_deps_accumulators_commute_ranges_are_exact_and_a_covering_write_supersedes():
    A, B, buf = "A", "B", ("buf", 1)
    read = lambda space, lo, hi: ([(space, lo, hi)], [], [])
    write = lambda space, lo, hi: ([], [(space, lo, hi)], [])
    acc = lambda space, lo, hi: ([], [], [(space, lo, hi)])
    cases = [                                   # (access, the earlier nodes it must follow)
        (write(A, 0, 1), set()),
        (acc(A, 0, 1), {0}),
        (acc(A, 0, 1), {0}),                    # accumulators do not follow each other
        (read(A, 0, 1), {0, 1, 2}),             # a read follows the last writer and every accumulator since
        (acc(A, 0, 1), {0, 3}),                 # an accumulate follows the last writer and every reader since
        (write(A, 0, 1), {0, 1, 2, 3, 4}),      # a write follows all three ...
        (read(B, 0, 1), set()),                 # (another space)
        (read(A, 0, 1), {5}),                   # ... and supersedes the history it covers
        (write(buf, 0, 4), set()),
        (write(buf, 4, 8), set()),              # disjoint channel ranges do not conflict
        (read(buf, 2, 6), {8, 9}),
        (read(buf, 8, 9), set()),               # half-open: [8, 9) touches neither writer
        (write(buf, 0, 8), {8, 9, 10}),         # node 11 read outside the range
        (read(buf, 3, 5), {12}),                # the covering write superseded nodes 8 and 9
    ]
    assert _sched.hazard_deps([a for a, _ in cases]) == [d for _, d in cases]
