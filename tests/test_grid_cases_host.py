"""CPU tests of tests/_grid_cases.py: the shapes of tests/test_gpu_fused_grids.py reach a third, ragged workgroup in x and a
group at a row end in every family and layout; the owner of an element agrees with a brute-force walk of the slots; the reduced
designs hold every pair of values; and, for the seeded inputs of the reference cases, the eager float32 oracle is itself within
the tolerances of the float64 reference (a GPU failure is then not the input's fault)."""
import numpy as np
import pytest
import torch

import _grid_cases as gc
import _linearize_refs as lr
from _side_refs import video_stats_f64
from _util import assert_parity

SHAPE_OF = {f: (gc.S2 if f.startswith("linearize") else (gc.S1_CODE if f == "stats_multi" else gc.S1)) for f in gc.FAMILIES}
CASES = [(f, lay) for f in gc.FAMILIES for lay in gc.layouts_of(f)]
# the counts the module docstring of the GPU tests quotes: (slots or threads in x, workgroups)
QUOTED = {("merge_ingest", "nchw"): (676, 3), ("merge_ingest", "nhwc"): (1350, 6), ("merge_dark", "nchw"): (684, 3),
          ("merge_dark_ingest", "nchw"): (684, 3), ("merge_dark_ingest", "nhwc_bgr"): (1368, 6), ("stats_ingest", "nchw"): (674, 3),
          ("stats_ingest", "nhwc"): (2698, 11), ("stats_multi", "nchw"): (2130, 9), ("stats_multi", "nhwc"): (2130, 9),
          ("linearize_dark", "nchw"): (2211, 3), ("linearize_dark_ingest", "nhwc"): (2211, 3), ("linearize_ingest", "nchw"): (2196, 3),
          ("linearize_ingest", "nhwc_bgr"): (2196, 3)}


@pytest.mark.parametrize("family,layout", CASES)
def test_shapes_meet_the_three_conditions(family, layout):
    h, w = SHAPE_OF[family]
    assert w % 2 == 1
    got = gc.conditions(family, layout, h, w)
    assert got["workgroups"] >= 3 and got["ragged"] and got["row_end"] in (True, None), got
    # no row-end condition only where a thread owns ONE pixel: the interleaved statistics ingest
    assert (got["row_end"] is None) == (family == "stats_ingest" and layout != "nchw")
    if (family, layout) in QUOTED:
        assert (gc.slots_x(family, layout, h, w)[0], got["workgroups"]) == QUOTED[(family, layout)]


def test_code_form_statistics_run_packets_only_where_the_frame_stride_allows():
    """stats_frames_vec_ok: ct_video_stats_batches hands over image_stride = C H W, so 3x38x71 (8094 = 2 mod 4) runs the V = 1
    kernel on every element -- 32 ragged workgroups, no vector body -- and 3x40x71 the V = 4 kernel on every element, no tail;
    so does the band [5, 33) of it."""
    assert not gc.stats_frames_vec_ok(3, *gc.S1) and gc.stats_frames_vec_ok(3, *gc.S1_CODE) and gc.stats_frames_vec_ok(3, 28, 71)
    assert not gc.stats_frames_vec_ok(3, *gc.S1_CODE, state_lead=1) and not gc.stats_frames_vec_ok(3, *gc.S1_CODE, frames_lead=2)
    for layout in gc.LAYOUTS:
        scalar = gc.conditions("stats_multi", layout, *gc.S1)
        assert gc.slots_x("stats_multi", layout, *gc.S1) == (8094, 256) and scalar == dict(workgroups=32, ragged=True, row_end=None)
        assert gc.slots_x("stats_multi", layout, *gc.S1_CODE) == (2130, 256) and (3 * 40 * 71) % 4 == 0
        assert gc.conditions("stats_multi", layout, *gc.S1_CODE) == dict(workgroups=9, ragged=True, row_end=True)
    assert gc.owner("stats_multi", "nchw", (3,) + gc.S1_CODE, 2, 39, 70) == 8
    assert gc.owner("stats_multi", "nchw", (3,) + gc.S1, 2, 37, 70) == 31
    assert gc.owner("stats_multi", "nhwc_bgr", (3,) + gc.S1_CODE, 2, 0, 0) == 0 and gc.owner("stats_multi", "nhwc", (3,) + gc.S1_CODE, 0, 39, 70) == 8


@pytest.mark.parametrize("family,layout", CASES)
def test_row_bands_still_have_a_second_ragged_workgroup(family, layout):
    """The bands the issue sets ([5, 33) of 38 rows, [9, 58) of 67) are shorter than three workgroups in some families: their
    cases are compared with the rows of the whole-image run, which has them all."""
    (r0, r1), (_, w) = (gc.BAND2 if family.startswith("linearize") else gc.BAND1), SHAPE_OF[family]
    got = gc.conditions(family, layout, r1 - r0, w)
    assert got["workgroups"] >= 2 and got["ragged"] and got["row_end"] in (True, None), got


def test_the_flat_forms_of_lin_typed():
    """ct_linearize_std_flat goes through lin_typed's own grids (tests/_linearize_refs.py restates the choice).  3x67x131 has
    Q = 26331, no multiple of 4: every frame goes element by element.  At 3x72x131 with aligned outputs the planar, the RGB
    and the packet8 kernel run, each on every element, with more than three workgroups and a ragged last one."""
    c, w = 3, gc.S2[1]
    at = lambda lead: {"lin": 4 * lead, "std_out": 4 * lead}   # noqa: E731
    h = gc.S2[0]
    q = c * h * w
    for lead in (0, 1, 2, 3):
        for layout, std in (("nchw", "multiplier"), ("nhwc", "none"), ("nhwc_bgr", "explicit")):
            assert lr.linearize_path_of("u8", layout, c, h * w, q, 3, std, at(lead), (q, q)) == "scalar"
    assert -(-q // 256) == 103 and q % 256 != 0
    h = gc.S2_STD[0]
    q = c * h * w
    assert w % 2 == 1 and q % 8 == 0
    assert lr.linearize_path_of("u16", "nchw", c, h * w, q, 3, "multiplier", at(0), (q, q)) == "planar"
    assert lr.linearize_path_of("f32", "nhwc_bgr", c, h * w, q, 3, "constant", at(0), (q, q)) == "rgb"
    assert lr.linearize_path_of("u8", "nhwc", c, h * w, q, 3, "explicit", at(0), (q, q)) == "packet8"
    for threads, per_block in ((q, 3072), (h * w // 4, 256), (q, 2048)):      # planar, RGB (4 pixels per thread), packet8
        assert -(-threads // per_block) >= 3 and threads % per_block != 0
    assert (-(-q // 3072), -(-(h * w // 4) // 256), -(-q // 2048)) == (10, 10, 14)
    assert gc.lin_typed_owner("planar", (c, h, w), "nchw", 2, h - 1, w - 1) == 9
    assert gc.lin_typed_owner("planar+tail", (c, 67, w), "nchw", 2, 66, w - 1) == "tail launch"
    assert gc.lin_typed_owner("rgb", (c, h, w), "nhwc_bgr", 1, h - 1, w - 1) == 9 and gc.lin_typed_owner("rgb", (c, h, w), "nhwc", 0, 7, 107) == 1
    assert gc.lin_typed_owner("packet8", (c, h, w), "nhwc", 1, 9, 0) == (9 * w * 3 + 1) // 2048 and gc.lin_typed_owner("packet8", (c, h, w), "nhwc", 2, h - 1, w - 1) == 13
    assert gc.lin_typed_owner("scalar", (c, 67, w), "nhwc_bgr", 0, 66, w - 1) == 102


@pytest.mark.parametrize("family,layout", CASES)
def test_owner_agrees_with_a_walk_of_the_slots(family, layout):
    """Every element has one owner, the owners are the workgroups 0 .. grid_x - 1 and each is used (lead 0 and 1)."""
    h, w = SHAPE_OF[family]
    for lead in (0, 1):
        seen = set()
        for c in range(3):
            for row in range(h):
                for col in (0, 1, 2, 3, w // 2, w - 4, w - 3, w - 2, w - 1):
                    seen.add(gc.owner(family, layout, (3, h, w), c, row, col, 0, lead))
        groups = {s for s in seen if not isinstance(s, str)}
        assert groups == set(range(gc.grid_x(family, layout, h, w))), (lead, sorted(groups, key=str))


def test_where_differs_names_the_place():
    h, w = gc.S1
    a = np.zeros((3, h, w), dtype=np.float32)
    assert gc.where_differs(a, a.copy(), "merge_dark", "nchw") is None
    b = a.copy()
    b[1, 30, 69] = 1.0
    b[2, 0, 0] = -0.0          # a bit pattern, not a value
    msg = gc.where_differs(b, a, "merge_dark", "nchw")
    flat = (1 * h + 30) * w + 69
    assert f"flat index {flat} = (frame 0, channel 1, row 30, column 69)" in msg and "2 of" in msg
    assert f"x-workgroup {(30 * 18 + 17) // 256} of merge_dark" in msg
    four = np.zeros((2, 3, h, w))
    other = four.copy()
    other[1, 0, 2, 5] = 3.0
    assert "(frame 1, channel 0, row 2, column 5)" in gc.where_differs(other, four, "linearize_dark", "nchw")


def test_designs_hold_every_pair():
    assert gc.pairs_covered(gc.merge_ingest_design(), ("u8", "u16"), gc.LAYOUTS, gc.INTERPS, gc.STDS)
    assert gc.pairs_covered(gc.merge_dark_design(), gc.DTYPES, gc.INTERPS, gc.STDS)
    assert gc.pairs_covered(gc.merge_dark_ingest_design(), gc.DTYPES, gc.LAYOUTS, gc.INTERPS, gc.STDS)
    assert gc.pairs_covered(gc.stats_design("code"), gc.DTYPES, gc.LAYOUTS, gc.INTERPS)
    assert gc.pairs_covered(gc.stats_design("ingest"), ("u8", "u16"), gc.LAYOUTS, gc.INTERPS)
    assert gc.pairs_covered(gc.linearize_ingest_design(), gc.DTYPES, gc.LAYOUTS, gc.INTERPS, gc.STDS, allowed=gc._no_lookup_std)
    assert gc.pairs_covered(gc.linearize_dark_design(gc.LAYOUTS), gc.DTYPES, gc.LAYOUTS, (None, "linear", "catmull"), gc.STDS)
    assert not any(t[2] == "lookup" and t[3] != "none" for t in gc.linearize_ingest_design())
    assert len(gc.merge_dark_ingest_design()) < 3 * 3 * 4 * 4 // 4      # a reduced design, not the product
    assert not gc.pairs_covered(gc.merge_dark_design()[:-1], gc.DTYPES, gc.INTERPS, gc.STDS)    # (the check bites)
    for design, layout_at in ((gc.stats_design("code"), 1), (gc.stats_design("ingest"), 1), (gc.linearize_dark_design(gc.LAYOUTS), 1)):
        assert {t[layout_at] for t in design} == set(gc.LAYOUTS)
    for lay in gc.LAYOUTS:      # the dark linearize forms pick their reference case among the LINEAR ones of a layout
        assert any(t[1] == lay and t[2] == "linear" for t in gc.linearize_dark_design(gc.LAYOUTS))
    assert any(t[2] == "linear" for t in gc.linearize_dark_design(("nchw",)))


def test_chain_f32_is_float32_arithmetic():
    codes = gc.random_codes(1, (2, 3, 4, 5), "u16")
    stages = gc.black_level_stages("u16")
    got = gc.chain_f32(codes, stages)
    x = torch.from_numpy(codes.astype(np.float32))
    want = ((x - np.float32(stages[0][1])) / np.float32(stages[0][2])) * 1.0 + 0.0
    assert got.dtype == np.float32 and np.array_equal(got, want.numpy())
    lo_hi = gc.chain_f32(codes, stages + [("clamp", [(0.1, 0.9)])])
    assert lo_hi.min() == np.float32(0.1) and lo_hi.max() == np.float32(0.9)
    data = gc.chain_f32(codes, [("affine_data", 1.0, 0.0)], consts=(np.float32(16.0), np.float32(1000.0)))
    assert np.array_equal(data, ((x - 16.0) / 1000.0).numpy())
    assert gc.to_layout(codes, "nhwc_bgr")[1, 2, 3, 0] == codes[1, 2, 2, 3]


# ---- the references alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp,gauss,std", [("linear", True, "multiplier"), ("linear", False, "constant"), (None, False, "constant")])
def test_merge_oracles_agree_on_the_scene(interp, gauss, std):
    """oracle.eager_torch.merge_stack (float32, autograd) against oracle.ct_oracle (float64 closed form) on the scene of
    test_merge_ingest_against_the_float64_oracle, at its tolerances."""
    from oracle import ct_oracle as oc
    from oracle import eager_torch as oe
    planar, t = gc.scene_codes(17, 5, (3,) + gc.S1, "u16")
    pixels = gc.chain_f32(planar, gc.black_level_stages("u16"))
    sd = gc.sigma_of(std, pixels, None)
    lut = gc.lut()
    mean_o, std_o = oc.hdr_merge(pixels, sd, t, None if interp is None else lut, interp or "none", gauss)
    mean_e, std_e = oe.merge_stack(torch.from_numpy(pixels), torch.from_numpy(sd), torch.from_numpy(t),
                                   None if interp is None else torch.from_numpy(lut), interp or "linear", gauss)
    assert_parity(mean_e.numpy(), mean_o, rtol=1e-5, norm_tol=1e-6, what="eager merge mean vs float64")
    assert_parity(std_e.numpy(), std_o, rtol=1e-5, norm_tol=1e-5, what="eager merge std vs float64")


@pytest.mark.parametrize("form,k", [(form, min(k for k, t in enumerate(gc.stats_design(form)) if t[1] == lay))
                                    for form in ("ingest", "code") for lay in gc.LAYOUTS])
def test_statistics_oracles_agree_on_the_reference_cases(form, k):
    from oracle import eager_torch as oe
    dtype, _, interp = gc.stats_design(form)[k]
    planar = gc.random_codes(600 + k, (7, 3) + (gc.S1 if form == "ingest" else gc.S1_CODE), dtype)
    pixels = gc.chain_f32(planar, gc.black_level_stages(dtype)) if form == "ingest" else lr.to_pixels(planar, dtype, gc.TOP[dtype])
    lut = gc.lut()
    mean_o, std_o = video_stats_f64(lr.linearize_f64(pixels, None, lut, interp)[0], [7])
    mean_e, std_e = oe.video_mean_std(torch.from_numpy(pixels), None if interp is None else torch.from_numpy(lut), interp, [3, 2, 2])
    assert_parity(mean_e.numpy(), mean_o, rtol=1e-6, norm_tol=1e-7, what="eager video mean vs float64")
    assert_parity(std_e.numpy(), std_o, rtol=1e-4, norm_tol=1e-6, what="eager video std vs float64")


@pytest.mark.parametrize("case", gc.linearize_ingest_design(), ids=str)
def test_linearize_oracles_agree(case):
    """oracle.eager_torch.linearize_frame against _linearize_refs.linearize_f64 on the inputs of every case test_linearize_ingest
    sends to ``lr.check`` (no model: the value is a copy and |1 * sigma| the float32 sigma itself)."""
    from oracle import eager_torch as oe
    dtype, _, interp, std = case
    k = gc.linearize_ingest_design().index(case)
    planar = gc.random_codes(700 + k, (3, 3) + gc.S2, dtype)
    pixels = gc.chain_f32(planar, gc.black_level_stages(dtype))
    sigma = gc.sigma_of(std, pixels, gc.explicit_sigma(700 + k, planar.shape))
    lut = gc.lut()
    lin_o, std_o = lr.linearize_f64(pixels, sigma, lut, interp)
    if interp is None:
        assert np.array_equal(lin_o, pixels.astype(np.float64))
        lr.check(np.zeros_like(pixels) if sigma is None else np.abs(sigma), std_o, ("std", None), f"sigma {case}")
        return
    for f in range(3):
        lin_e, std_e = oe.linearize_frame(torch.from_numpy(pixels[f]), None if sigma is None else torch.from_numpy(sigma[f]),
                                          torch.from_numpy(lut), interp)
        lr.check(lin_e.numpy(), lin_o[f], ("lin", interp), f"eager linearize {case} lin")
        if sigma is not None:
            lr.check(std_e.numpy(), std_o[f], ("std", interp), f"eager linearize {case} std")
        else:
            assert not std_o[f].any()


# ---- the dark references ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["merge_dark", "merge_dark_ingest"])
def test_dark_merge_oracles_agree_on_the_scene(family):
    """oracle.eager_torch.merge_stack_dark (float32, autograd through the blur) on the inputs of
    test_dark_merges_against_the_eager_restatement, against float64: _side_refs.dark_blur_f64, then oracle.ct_oracle's closed-form
    merge on (xb, sigma_eff) with the same partition [3, 2] -- at the tolerances the GPU test applies."""
    from _side_refs import dark_blur_f64
    from oracle import ct_oracle as oc
    from oracle import eager_torch as oe
    h, w = gc.S1
    dtype = "f32" if family == "merge_dark" else "u16"
    planar, t = gc.scene_codes(23, 5, (3, h, w), dtype)
    pixels = gc.chain_f32(planar, gc.black_level_stages(dtype) if family == "merge_dark_ingest" else [])
    sigma = gc.explicit_sigma(23, planar.shape)
    dark, dark_std = gc.dark_fields(23, (1, 3, h, w))
    lut = gc.lut()
    xb, sig_eff = dark_blur_f64(pixels, dark, dark_std, sigma)
    mean_o, std_o = oc.hdr_merge(xb, sig_eff, t, lut, "linear", True, partition=[3, 2])
    mean_e, std_e = oe.merge_stack_dark(torch.from_numpy(pixels), torch.from_numpy(sigma), torch.from_numpy(t), torch.from_numpy(lut),
                                        torch.from_numpy(dark[0]), torch.from_numpy(dark_std[0]), "linear", True, [3, 2])
    assert_parity(mean_e.numpy(), mean_o, rtol=1e-5, norm_tol=1e-6, what=f"eager {family} mean vs float64")
    assert_parity(std_e.numpy(), std_o, norm_tol=1e-5, elem_tol=1e-5, what=f"eager {family} std vs float64")


def _lin_dark_reference_cases():
    """(form, case index, dtype, layout, std) of the cases test_linearize_dark sends to the eager restatement: the first LINEAR
    case of every form and layout."""
    out = []
    for form, layouts in (("dark", ("nchw",)), ("dark_ingest", gc.LAYOUTS)):
        design = gc.linearize_dark_design(layouts)
        for lay in layouts:
            k = min(i for i, t in enumerate(design) if t[1] == lay and t[2] == "linear")
            out.append((form, k, design[k][0], lay, design[k][3]))
    return out


@pytest.mark.parametrize("form,k,dtype,layout,std", _lin_dark_reference_cases())
def test_dark_linearize_oracles_agree(form, k, dtype, layout, std):
    """oracle.eager_torch.linearize_frame_dark on the inputs of test_linearize_dark's reference cases, against float64:
    _side_refs.dark_blur_f64, then _linearize_refs.linearize_f64 on (xb, sigma_eff) -- at the tolerances the GPU test applies."""
    from _side_refs import dark_blur_f64
    from oracle import eager_torch as oe
    planar = gc.random_codes(800 + k, (3, 3) + gc.S2, dtype)
    sigma = gc.explicit_sigma(800 + k, planar.shape)
    dark, dark_std = gc.dark_fields(800 + k, planar.shape)
    pix = gc.chain_f32(planar, gc.black_level_stages(dtype)) if form != "dark" else lr.to_pixels(planar, dtype, gc.TOP[dtype])
    sig = gc.sigma_of(std, pix, sigma)
    sig = np.zeros_like(pix) if sig is None else sig
    lut = gc.lut()
    xb, sig_eff = dark_blur_f64(pix, dark, dark_std, sig)
    lin_o, std_o = lr.linearize_f64(xb.astype(np.float32), sig_eff.astype(np.float32), lut, "linear")
    for f in range(3):
        lin_e, sd_e = oe.linearize_frame_dark(torch.from_numpy(pix[f]), torch.from_numpy(sig[f]), torch.from_numpy(lut),
                                              torch.from_numpy(dark[f]), torch.from_numpy(dark_std[f]), "linear")
        assert_parity(lin_e.numpy(), lin_o[f], rtol=1e-5, norm_tol=1e-6, what=f"eager linearize {form} {layout} value vs float64")
        assert_parity(sd_e.numpy(), std_o[f], rtol=1e-5, norm_tol=1e-6, what=f"eager linearize {form} {layout} std vs float64")
