"""Cases for the outline triangles (include/bs_api.h, "outline triangles"): the named cases and tolerances of
tests/uncross_ref/cases.py by import, and shapes of the stage's own, each with the tolerances it runs at."""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


uc = _load("uncross_cases", os.path.join(HERE, "..", "uncross_ref", "cases.py"))
tref = _load("triangulate_ref", os.path.join(HERE, "triangulate_ref.py"))
brute, uref, sc = tref.brute, tref.uref, uc.sc

TOLERANCES = uc.TOLERANCES
# the one run of the named cases with a hole that finds no bridge ("Outline triangles"): (name, tolerance, label)
NO_BRIDGE_RUNS = (("random_0", (10 ** 6, 1), 0),)


def comb(teeth):
    """a spine with `teeth` one-pixel teeth: 4 teeth + 4 vertices at tolerance 0, and an ear scan that really walks"""
    lab = np.full((3, 2 * teeth + 1), -1, np.int32)
    lab[0, :] = 0
    lab[1:, 1::2] = 0
    return sc._c(lab, 7)


def sieve(n, step, diagonal=False):
    """n x n of label 0 with one-pixel holes of label -1 every `step` pixels; diagonal: every second hole gets a
    neighbour that touches it at a corner (all but the last: 24, 3 gives 49 + 15 = 64 holes)"""
    lab = np.zeros((n, n), np.int32)
    lab[2:n - 1:step, 2:n - 1:step] = -1
    if diagonal:
        lab[3:n - 1:2 * step, 3:n - 1:2 * step] = -1
        lab[n - 3, n - 3] = 0
    return sc._c(lab, 8)


def blocked_nearest():
    """a hole at (6, 6) whose two nearest candidates, the corners (10, 3) and (11, 3) of a notch in the upper edge, lie
    behind the hole at (8, 4), which is not merged yet when it is taken: the bridge goes to the third nearest"""
    lab = np.zeros((10, 16), np.int32)
    lab[0:3, 10] = -1
    lab[6, 6] = -1
    lab[4, 8] = -1
    return sc._c(lab, 9)


def equal_left():
    """two holes with equal leftmost x"""
    lab = np.zeros((9, 7), np.int32)
    lab[2, 2:4] = -1
    lab[5:7, 2] = -1
    return sc._c(lab, 10)


def pinched():
    """3 x 3 without its centre and a corner: one ring through outside and hole that visits a corner twice"""
    return sc._c(np.array([[0, 0, 0], [0, -1, 0], [0, 0, -1]]), 11)


def two_outers():
    """label 0 in two pieces, each with a hole"""
    lab = np.full((7, 13), -1, np.int32)
    lab[1:6, 1:6] = 0
    lab[1:6, 7:12] = 0
    lab[3, 3] = lab[3, 9] = 1
    return sc._c(lab, 12)


def nested():
    """a label in the hole of a label in a hole"""
    lab = np.zeros((13, 13), np.int32)
    lab[2:11, 2:11] = 1
    lab[4:9, 4:9] = 2
    lab[6, 6] = 3
    return sc._c(lab, 13)


def long_comb():
    """one comb long enough to leave the LDS path at tolerance 0: more than LDS_CAP occurrences"""
    return comb(tref.LDS_CAP // 4 + 1)


def own_shapes():
    """name -> (case, tolerances)"""
    few = ((0, 1), (2, 1), (10 ** 6, 1))
    return {"comb_300": (comb(300), ((0, 1),)), "sieve_24": (sieve(24, 3, True), few[::2]), "sieve_30": (sieve(30, 4), few[::2]),
            "blocked_nearest": (blocked_nearest(), few), "equal_left": (equal_left(), few), "pinched": (pinched(), few),
            "two_outers": (two_outers(), few), "nested": (nested(), few), "long_comb": (long_comb(), ((0, 1),))}


def all_runs():
    """(name, case, (num, den)) of everything the suites run"""
    for name, c in uc.named_cases():
        for tol in TOLERANCES:
            yield name, c, tol
    for name, (c, tols) in own_shapes().items():
        for tol in tols:
            yield name, c, tol
