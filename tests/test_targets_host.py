"""CPU tests (no GPU) of the ground-truth plan's oracle (tests/targets_ref.py): it equals the torch spelling of the plan
(modeling/fcos.py: assign_targets, source_node_index, centerness_targets) bit for bit on the golden batch and on every edge case,
every case really sits on the comparison it is named for, the node-sampling indices stay in range, and the three entry points of
scan_amd/csrc/targets.hip refuse bad arguments before they touch a device."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import targets_ref as R
from scan_amd import _lib, ops, synth
from scan_amd.modeling import fcos

CPU = torch.device("cpu")


def _torch_plan(case):
    """the torch spelling on the CPU: labels, reg targets on every row, node index / labels, positives and their targets"""
    shape = ops.PyramidShape(case.N, case.sizes)
    labels, reg = fcos.assign_targets(fcos.compute_locations(shape, CPU, case.strides), case.torch_targets())
    idx, labs = fcos.source_node_index(labels, shape)
    pos = torch.nonzero(labels > 0).squeeze(1)
    return labels, reg, idx, labs, pos, reg[pos], fcos.centerness_targets(reg[pos])


def _assert_oracle_equals_torch(case):
    labels, reg, idx, labs, pos, reg_pos, ctr = _torch_plan(case)
    assert np.array_equal(case.labels, labels.numpy())
    assert np.array_equal(case.reg.view(np.int32), reg.numpy().view(np.int32))  # every row, not only the positives
    want = case.nodes
    assert np.array_equal(want["node_index"], idx.numpy()) and np.array_equal(want["node_labels"], labs.numpy())
    assert np.array_equal(want["pos_inds"], pos.numpy())
    assert np.array_equal(want["reg_pos"].view(np.int32), reg_pos.numpy().view(np.int32))
    assert np.array_equal(want["ctr_pos"].view(np.int32), ctr.numpy().view(np.int32))
    assert [int(v) for v in want["level_pos"]] == case.counts["level_pos"]


@pytest.mark.parametrize("name", R.PLAN_CASES)
def test_oracle_equals_the_torch_spelling(name):
    _assert_oracle_equals_torch(R.case(name))


def test_oracle_equals_the_torch_spelling_and_the_goldens_on_the_golden_batch(gold_dir):
    gold = json.load(open(os.path.join(gold_dir, "step_128x256.json")))
    g = np.load(os.path.join(gold_dir, "step_128x256.npz"))
    H, W, N = gold["H"], gold["W"], gold["N"]
    case = R.case_from_targets("golden", H, W, [(b.numpy(), l.numpy()) for b, l in synth.synth_targets(N, H, W, 8, 12, 4321)])
    _assert_oracle_equals_torch(case)
    for l in range(5):
        assert np.array_equal(case.labels[case.shape.row_off[l]:case.shape.row_off[l + 1]], g["label_map_%d" % l])
    assert np.array_equal(case.nodes["node_labels"], g["node_labels"])
    assert case.counts["n_nodes"] > 0 and sum(case.counts["level_pos"]) > 0


def test_locations_are_the_module_s():
    sizes = R.pyramid_sizes(96, 160)
    for got, want in zip(R.locations(sizes, R.STRIDES), fcos.compute_locations(ops.PyramidShape(1, sizes), CPU)):
        assert got.dtype == np.float32 and np.array_equal(got, want.numpy())


# ----------------------------------------------------------------------------- every case sits where its name says
def test_ties_case_counts_and_first_minimum_rule():
    c, rev = R.case("ties"), R.case("ties_reversed")
    n = c.counts
    assert (n["tie_rows"], n["mx_eq_lo"], n["mx_eq_hi"], n["mn_eq_0"]) == (66, 16, 32, 96), n
    assert n["level_pos"] == [62, 16, 0, 0, 0]
    assert n["tie_rows"] >= 50 and n["mx_eq_lo"] >= 10 and n["mx_eq_hi"] >= 10 and n["mn_eq_0"] >= 50
    assert n["mn_eq_0_in_range"] > 0  # ... where the strict ``mn > 0`` alone decides
    # the same boxes in the opposite order: the rows with a tie, and only they, change their label -- the order decided them
    ties = R.tie_rows(c.sizes, c.N, c.boxes, c.ng)
    assert np.array_equal(ties, R.tie_rows(rev.sizes, rev.N, rev.boxes, rev.ng)) and int(ties.sum()) == 66
    assert (c.labels[ties] != rev.labels[ties]).all() and np.array_equal(c.labels[~ties], rev.labels[~ties])
    assert 5 not in c.labels and 2 not in rev.labels  # of the two equal boxes the later one never wins
    assert rev.counts == c.counts


def test_integer_grid_case_counts():
    n = R.case("integer_grid").counts
    assert n["mn_eq_0"] >= 100 and n["mx_eq_hi"] >= 20, n
    assert (n["mn_eq_0"], n["mx_eq_hi"], n["mx_eq_lo"]) == (221, 33, 11), n  # seed 7 of numpy's RandomState
    assert n["mn_eq_0_in_range"] >= 20
    b = R.case("integer_grid").boxes
    assert np.array_equal(b % 4, np.zeros_like(b)) and b[..., 2].max() <= 256 and b[..., 3].max() <= 128


def test_counts_of_the_small_cases():
    assert R.case("zero_positives").counts["level_pos"] == [0, 0, 0, 0, 0] and R.case("zero_positives").counts["n_nodes"] == 0
    assert R.case("one_positive").counts["level_pos"] == [1, 0, 0, 0, 0] and R.case("one_positive").counts["n_nodes"] == 2
    c = R.case("covers_everything")  # both rows of the coarsest level positive: np = 2 > nn = 0 there
    assert c.counts["level_pos"] == [0, 0, 0, 0, 2] and c.shape.row_off[5] - c.shape.row_off[4] == 2 and c.counts["n_nodes"] == 2
    assert R.case("few_levels_1").shape.n_levels == 1 and R.case("few_levels_3").shape.n_levels == 3
    for name in ("few_levels_1", "few_levels_3"):
        c = R.case(name)
        assert all(v > 0 for v in c.counts["level_pos"]) and c.counts["mn_eq_0"] >= 100 and c.counts["mx_eq_hi"] >= 20
        assert len(c.strides) == len(c.soi) == c.shape.n_levels
        # the truncated pyramid is the head of the full one
        full = R.case("integer_grid")
        assert np.array_equal(c.labels, full.labels[:c.shape.rows]) and np.array_equal(c.reg, full.reg[:c.shape.rows])


def test_ragged_case_never_reads_a_padded_slot():
    c = R.case("ragged_with_empty_image")
    assert list(c.ng) == [4, 0, 1] and c.G == 7 and not c.all_images_have_boxes
    for n in range(3):
        assert np.isnan(c.boxes[n, c.ng[n]:]).all() and (c.glabels[n, c.ng[n]:] == 999).all()
        assert not np.isnan(c.boxes[n, :c.ng[n]]).any()
    assert not (c.labels == 999).any() and not np.isnan(c.reg).any()
    assert c.counts["tie_rows"] == 66 and all(v > 0 for v in c.counts["level_pos"][:3])
    for l, (h, w) in enumerate(c.sizes):  # the image without boxes: label 0, zero targets
        r0 = c.shape.row_off[l] + h * w
        assert (c.labels[r0:r0 + h * w] == 0).all() and (c.reg[r0:r0 + h * w] == 0).all()
    # image 0 is the ties case: the same labels and targets, whatever the other images and the padding hold
    t = R.case("ties")
    for l, (h, w) in enumerate(c.sizes):
        a, b = c.shape.row_off[l], t.shape.row_off[l]
        assert np.array_equal(c.labels[a:a + h * w], t.labels[b:b + h * w]) and np.array_equal(c.reg[a:a + h * w], t.reg[b:b + h * w])


def test_synthetic_label_vectors_reach_every_count_combination():
    """tests/test_gpu_targets.py drives the compaction and node kernels with these: each level size with each pattern, and the
    count relations the node kernel branches on are all present"""
    seen_sizes, seen, relations = set(), set(), set()
    for sizes, labels, reg, names in R.label_cases():
        shape = R.Shape(1, sizes)
        assert len(labels) == shape.rows and reg.shape == (shape.rows, 4) and (reg > 0).all()
        per_level = []
        for l, (p, n) in enumerate(R.compact(labels, shape.row_off)):
            rows = shape.row_off[l + 1] - shape.row_off[l]
            assert len(p) + len(n) == rows
            seen_sizes.add(rows)
            seen.add((rows, names[l]))
            per_level.append(len(p))
            for rel, hit in (("np==0", len(p) == 0), ("nn==0", len(n) == 0), ("np==1", len(p) == 1), ("nn==1", len(n) == 1),
                             ("np==nn", len(p) == len(n)), ("np==nn+1", len(p) == len(n) + 1), ("np==nn-1", len(p) == len(n) - 1),
                             ("np>nn+1", len(p) > len(n) + 1), ("1<np<nn-1", 1 < len(p) < len(n) - 1)):
                if hit:
                    relations.add(rel)
            for k in (0, 63, 64, 1023, 1024, rows - 1):  # a lone positive at a wave / 1024-row boundary
                if len(p) == 1 and p[0] - shape.row_off[l] == k:
                    relations.add("lone@%s" % ("last" if k == rows - 1 and k not in (0, 63, 64, 1023, 1024) else k))
        if len(per_level) >= 3 and any(per_level[i] == 0 and per_level[i - 1] > 0 and per_level[i + 1] > 0
                                       for i in range(1, len(per_level) - 1)):
            relations.add("empty level between others")
    assert seen_sizes == set(R.LEVEL_SIZES)
    assert seen >= {(r, p) for pyr in R.LABEL_PYRAMIDS for r in pyr for p in R.PATTERNS}
    assert relations >= {"np==0", "nn==0", "np==1", "nn==1", "np==nn", "np==nn+1", "np==nn-1", "np>nn+1", "1<np<nn-1", "lone@0",
                         "lone@63", "lone@64", "lone@1023", "lone@1024", "lone@last", "empty level between others"}, relations
    assert sum(1 for _, labels, _, _ in R.label_cases() if not (labels > 0).any()) >= 1  # the early return at zero nodes


# ----------------------------------------------------------------------------- node sampling indices
def test_linspace_picks_stay_in_range():
    pairs = [(p, n) for n in range(1, 301) for p in range(1, n + 1)]
    pairs += [(1, 1), (1, 2), (2, 2), (7, 51), (333, 1000), (999, 1000), (1000, 1000)]
    for p, n in pairs:
        idx = R.pick(p, n)
        top = max(n - 2, 0)
        assert len(idx) == p and idx[0] == 0
        assert (np.diff(idx) >= 0).all() and idx.min() >= 0 and idx.max() <= top, (p, n)
        if p > 1:
            assert idx[-1] == top, (p, n)
    assert np.array_equal(R.pick(3, 2), [0, 1]) and len(R.pick(0, 5)) == 0 and len(R.pick(2, 0)) == 0


# ----------------------------------------------------------------------------- argument validation, before any launch
def test_plan_entry_points_refuse_bad_arguments_without_a_device():
    L, fake = _lib.lib(), ctypes.c_void_p(4096)  # never dereferenced: every call below is refused first
    good = ops.PyramidShape(2, [(4, 4), (2, 2)])
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)

    def refused(rc, text):
        assert rc == -1 and re.search(text, L.scan_last_error().decode()), (rc, L.scan_last_error())

    def bad_pyramids():
        for n_levels, n_images in ((0, 1), (_lib.MAX_LEVELS + 1, 1)):
            d = _lib.PyramidDesc()
            d.n_levels, d.n_images = n_levels, n_images
            yield ctypes.byref(d)
        yield None

    # scan_fcos_nodes_count
    assert L.scan_fcos_nodes_count(None, i32(0, 0)) == -1 and L.scan_fcos_nodes_count(good.ref(), None) == -1
    assert L.scan_fcos_nodes_count(None, None) == -1
    assert L.scan_fcos_nodes_count(good.ref(), i32(0, 0)) == 0
    assert L.scan_fcos_nodes_count(good.ref(), i32(3, 8)) == 3 + 3 + 8 + 0  # np <= nn: np picks; np > nn: every background row
    for name in R.CASES:
        c = R.case(name)
        assert L.scan_fcos_nodes_count(ops.PyramidShape(c.N, c.sizes).ref(), i32(*c.counts["level_pos"])) == c.counts["n_nodes"]

    # scan_fcos_assign
    def assign(d=good.ref(), G=3, **null):
        a = {k: fake for k in ("strides", "soi", "boxes", "glabels", "ng", "labels", "labels_i32", "reg", "level_pos")}
        a.update(null)
        return L.scan_fcos_assign(d, a["strides"], a["soi"], a["boxes"], a["glabels"], a["ng"], G, a["labels"], a["labels_i32"],
                                  a["reg"], a["level_pos"], None)

    for d in bad_pyramids():
        refused(assign(d=d), "fcos_assign: bad pyramid")
    no_images = _lib.PyramidDesc()
    no_images.n_levels, no_images.n_images = 1, 0
    refused(assign(d=ctypes.byref(no_images)), "fcos_assign: bad pyramid")
    for k in ("strides", "soi", "boxes", "glabels", "ng", "labels", "labels_i32", "reg", "level_pos"):
        refused(assign(**{k: None}), "fcos_assign: null pointer or G < 1")
    for G in (0, -1):
        refused(assign(G=G), "fcos_assign: null pointer or G < 1")

    # scan_fcos_compact
    for d in bad_pyramids():
        refused(L.scan_fcos_compact(d, fake, fake, fake, None), "fcos_compact: bad pyramid")
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        refused(L.scan_fcos_compact(good.ref(), *args, None), "fcos_compact: null pointer")
    huge = ops.PyramidShape(1, [(46341, 46341)])  # 46341^2 = 2^31 + 4633: row indices would not fit the int32 lists
    assert huge.rows >= 2 ** 31
    refused(L.scan_fcos_compact(huge.ref(), fake, fake, fake, None), "2\\^31 rows")

    # scan_fcos_nodes
    def nodes(d=good.ref(), level_pos=i32(1, 0), outs=(fake,) * 5, **null):
        a = {k: fake for k in ("labels", "reg", "pos_list", "neg_list")}
        a.update(null)
        return L.scan_fcos_nodes(d, level_pos, a["labels"], a["reg"], a["pos_list"], a["neg_list"], *outs, None)

    for d in bad_pyramids():
        refused(nodes(d=d), "fcos_nodes: bad pyramid")
    refused(nodes(level_pos=None), "fcos_nodes: null pointer")
    for k in ("labels", "reg", "pos_list", "neg_list"):
        refused(nodes(**{k: None}), "fcos_nodes: null pointer")
    refused(nodes(level_pos=i32(33, 0)), "level 0 has 33 positives of 32 rows")
    refused(nodes(level_pos=i32(0, -1)), "level 1 has -1 positives of 8 rows")
    for i in range(5):  # with a node to write, every output is needed
        refused(nodes(outs=tuple(None if j == i else fake for j in range(5))), "fcos_nodes: null output")
    # ... and with none, the call returns before it looks at them (and before any launch)
    assert nodes(level_pos=i32(0, 0), outs=(None,) * 5) == 0


def test_plan_entry_points_refuse_an_inconsistent_pyramid_before_any_launch():
    """a level whose rows are not n_images * h * w would send the row decode past the images' box counts: every plan entry
    point checks the whole descriptor (scan_check_pyramid in csrc/common.h), not only its level count"""
    L, fake = _lib.lib(), ctypes.c_void_p(4096)  # never dereferenced
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)

    def broken(edit):
        s = ops.PyramidShape(2, [(4, 4), (2, 2)])
        edit(s.desc)
        return s

    def rows_off(d):
        d.row_off[1] += 1

    def no_height(d):
        d.h[1] = 0

    def more_images(d):
        d.n_images = 3

    for edit in (rows_off, no_height, more_images):
        s = broken(edit)
        for rc in (L.scan_fcos_assign(s.ref(), *(fake,) * 5, 3, *(fake,) * 4, None),
                   L.scan_fcos_compact(s.ref(), fake, fake, fake, None),
                   L.scan_fcos_nodes(s.ref(), i32(0, 0), *(fake,) * 9, None)):
            assert rc == -1 and re.search(r"fcos_\w+: level \d of the pyramid is inconsistent", L.scan_last_error().decode())
    huge = ops.PyramidShape(1, [(46341, 46341)])
    assert L.scan_fcos_assign(huge.ref(), *(fake,) * 5, 3, *(fake,) * 4, None) == -1
    assert "level 0 alone has 2^31 rows or more" in L.scan_last_error().decode()
