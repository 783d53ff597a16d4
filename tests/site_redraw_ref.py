"""Float64 restatement of arp_site_redraw, written from the contract in include/autoreparam.h.  Thin on purpose: a flagged
element is tests/prior_draw_ref.py's draw of that element from the parents the row holds, an unflagged one is the input;
the bound, the undecided attempts and what they taint are prior_draw_ref's, restricted to the flagged elements.

`redraw(table, x, flags, seed, offset, parents=None)` -> prior_draw_ref.Draws(x [R, D] float64, undrawn [R], terms)
    x: the recorded rows [R, D]; flags: [D], non-zero for an element that is redrawn.  With `parents` (the device's own
    float32 OUTPUT rows [R, D]: the redrawn value where the parent is flagged, the recorded one where it is not) every
    flagged element is computed from those parents -- teacher forcing, as in test_gpu_prior_draws.  Without, the reference
    builds the rows itself: it teacher-forces on its own rows, starting from 0 in the flagged columns, until they stop
    changing -- after pass p every flagged element whose flagged ancestors are at most p - 1 deep is final, so at most D
    passes; the accept test of the log-Gamma form reads no parent, so the attempts are the same in every pass.
`bound(table, d)`, `undecided(table, d, flags)`, `tainted(table, marks, flags)`: prior_draw_ref's, on the flagged columns
    (an undecided attempt of an unflagged element decides nothing; a taint is passed on through every term of non-zero
    weight, as there -- through an unflagged element too, which excludes more than it has to, never less)."""
import numpy as np

import prior_draw_ref as pr


def _forced(table, x, flagged, seed, offset, parents):
    d = pr.draw(table, x.shape[0], seed, offset, parents=parents)
    rows = np.where(flagged[None, :], d.x, x)
    gamma = (np.asarray(table.form).reshape(-1) == pr.LOG_GAMMA) & flagged
    return pr.Draws(rows, _ran_out(table, d, gamma), d.terms)


def _ran_out(table, d, gamma):
    """Draws one of whose FLAGGED log-Gamma elements (of a shape that can be drawn) found no accepting attempt"""
    k = np.asarray(table.loc0, np.float64).reshape(-1)
    can = gamma & np.isfinite(k) & (k > 0)
    return np.isnan(d.terms["t"][:, can]).any(axis=1) if can.any() else np.zeros(d.x.shape[0], bool)


def redraw(table, x, flags, seed, offset, parents=None):
    x = np.asarray(x, np.float64)
    flagged = np.asarray(flags).reshape(-1) != 0
    assert x.ndim == 2 and flagged.size == x.shape[1]
    if parents is not None:
        return _forced(table, x, flagged, seed, offset, np.asarray(parents, np.float64))
    rows = np.where(flagged[None, :], 0.0, x)
    for _ in range(x.shape[1] + 1):
        d = _forced(table, x, flagged, seed, offset, rows)
        if np.array_equal(d.x, rows, equal_nan=True):
            return d
        rows = d.x
    raise AssertionError("the rows did not settle in D passes: the table is not in ancestral order")


def bound(table, d):
    return pr.bound(table, d)


def undecided(table, d, flags):
    return pr.undecided(table, d) & (np.asarray(flags).reshape(-1) != 0)[None, :]


def tainted(table, marks, flags):
    return pr.tainted(table, marks) & (np.asarray(flags).reshape(-1) != 0)[None, :]
