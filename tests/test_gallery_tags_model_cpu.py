"""Pins tests/gallery_tags_model.py (the oracle of the tagged gallery queries) on hand-written cases of a few rows: no GPU."""
import numpy as np

from tests import gallery_tags_model as model

F = np.float32
NAN = np.float32("nan")


def f32(*rows):
    return np.array(rows, np.float32)


def test_an_excluded_best_row_is_not_listed_and_does_not_displace_anyone():
    sc = f32([0.9, 0.8, 0.7, 0.6])
    tags = [2, 1, 1, 3]
    s, r = model.topk_from_scores(sc, tags, [1], 2, base=10)
    assert r.tolist() == [[11, 12]] and s.tolist() == [[F(0.8), F(0.7)]]
    s, r = model.topk_from_scores(sc, tags, [2], 2, base=10)
    assert r.tolist() == [[10, 13]] and s.tolist() == [[F(0.9), F(0.6)]]
    s, r = model.topk_from_scores(sc, tags, [model.TAG_ALL], 4)
    assert r.tolist() == [[0, 1, 2, 3]]


def test_each_query_has_its_own_mask():
    sc = f32([0.9, 0.8, 0.1], [0.2, 0.3, 0.95])
    tags = [1, 2, 4]
    s, r = model.topk_from_scores(sc, tags, [6, 3], 3)
    assert r.tolist() == [[1, 2, -1], [1, 0, -1]]
    assert s.tolist() == [[F(0.8), F(0.1), F(-1.0)], [F(0.3), F(0.2), F(-1.0)]]


def test_ties_across_tags_go_to_the_lowest_admitted_index():
    sc = f32([0.5, 0.5, 0.5, 0.5])
    tags = [1, 2, 1, 2]
    assert model.topk_from_scores(sc, tags, [2], 2)[1].tolist() == [[1, 3]]
    assert model.topk_from_scores(sc, tags, [1], 2)[1].tolist() == [[0, 2]]
    assert model.topk_from_scores(sc, tags, [3], 3, base=5)[1].tolist() == [[5, 6, 7]]


def test_mask_zero_lists_nothing_and_labels_minus_one():
    sc = f32([0.9, 0.8])
    s, r = model.topk_from_scores(sc, [model.TAG_ALL, 1], [0], 3)
    assert r.tolist() == [[-1, -1, -1]] and s.tolist() == [[F(-1.0)] * 3]
    lab, best = model.label_from_scores(sc, [model.TAG_ALL, 1], [0], 0.0)
    assert lab.tolist() == [-1] and best.tolist() == [F(-1.0)]
    s, d, r = model.topk_ids_from_scores(sc, [4, 4], [1, 1], [0], 2)
    assert d.tolist() == [[-1, -1]] and r.tolist() == [[-1, -1]] and s.tolist() == [[F(-1.0)] * 2]


def test_fewer_admitted_rows_than_k_leave_the_tail_empty():
    sc = f32([0.1, 0.2, 0.3, 0.4, 0.5])
    s, r = model.topk_from_scores(sc, [8, 1, 8, 1, 1], [8], 4)
    assert r.tolist() == [[2, 0, -1, -1]] and s.tolist() == [[F(0.3), F(0.1), F(-1.0), F(-1.0)]]


def test_an_admitted_nan_row_is_never_listed():
    sc = f32([NAN, 0.2, NAN, 0.4])
    s, r = model.topk_from_scores(sc, [1, 1, 2, 2], [1], 2)
    assert r.tolist() == [[1, -1]] and s.tolist() == [[F(0.2), F(-1.0)]]
    lab, best = model.label_from_scores(f32([NAN, NAN]), [1, 1], [1], 0.0)
    assert lab.tolist() == [-1] and best.tolist() == [F(-1.0)]


def test_an_identity_is_represented_by_its_best_admitted_template():
    #             id 7: rows 0 (best, excluded), 2        id 9: rows 1, 3 (excluded)
    sc = f32([0.9, 0.6, 0.5, 0.8])
    ids, tags = [7, 9, 7, 9], [2, 1, 1, 2]
    s, d, r = model.topk_ids_from_scores(sc, ids, tags, [1], 2, base=100)
    assert d.tolist() == [[9, 7]] and r.tolist() == [[101, 102]] and s.tolist() == [[F(0.6), F(0.5)]]
    s, d, r = model.topk_ids_from_scores(sc, ids, tags, [3], 2, base=100)          # all admitted: the best templates
    assert d.tolist() == [[7, 9]] and r.tolist() == [[100, 103]]
    s, d, r = model.topk_ids_from_scores(sc, ids, tags, [2], 3, base=100)
    assert d.tolist() == [[7, 9, -1]] and r.tolist() == [[100, 103, -1]]


def test_label_is_strict_and_names_the_identity_of_the_best_admitted_row():
    sc = f32([0.9, 0.6])
    lab, best = model.label_from_scores(sc, [2, 1], [1], 0.6)
    assert lab.tolist() == [-1] and best.tolist() == [F(0.6)]
    lab, best = model.label_from_scores(sc, [2, 1], [1], np.nextafter(F(0.6), F(0)), base=3)
    assert lab.tolist() == [4]
    lab, _ = model.label_from_scores(sc, [2, 1], [1], 0.1, base=3, ids=[50, 60])
    assert lab.tolist() == [60]


def test_admitted_matrix():
    a = model.admitted([0, 1, 0x80000000, model.TAG_ALL], [0x80000001, 0])
    assert a.tolist() == [[False, True, True, True], [False] * 4]
