"""CPU: the shape table of the general tile kernel (tests/general_shapes.py).

* the table covers resample.hip: every (VEC, C, F32, ALPHA) of ``launch_v`` /
  ``launch_resample`` / ``launch_t`` has its ``(VEC, C, ALPHA)`` frames, so an
  instantiation added without a shape fails here;
* tests/cpp/general_layout_unit.cpp (``build_layout`` in the device-free
  environment, under MXD_POLICY_NO_WAVE) tiles every launch the GPU test
  submits -- every frame's windows in every source layout, every named launch
  -- exactly as general_shapes.tiling / launch_cfg restate it: vec, tiles,
  tile_begin, LDS bytes, and per image strips, tx, ty, group, vw;
* every shape has the tiling it was committed for (one tile; strips with a
  short last one, two bands with a short last one, a row group shorter than
  the band), every named launch the property in its entry;
* the finder reproduces the committed table;
* on every frame of 64 x 64 and more the references agree within the
  project's gate: the kernel-order restatements against the stbir-order oracle
  within +-1 and 2e-3 differing channels, on the seeds the GPU test uses;
* for the deep ratios the product's tap tables are the oracle's, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import general_shapes as G
import oracle as O
import wave_shapes as W
from gpu_util import compare, oracle_out, synth
from mlx_data_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "mlx-data_amd")
HIPCC = "/opt/rocm/bin/hipcc"
MAX_FRAC = 2e-3
KEYS = sorted(G.SHAPES)

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def unit(tmp_path_factory):
    """launches [(f32, [mxd_image fields])] -> [(launch fields, [image fields]) or (rc, message)]."""
    exe = str(tmp_path_factory.mktemp("general_layout") / "general_layout_unit")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "-I", os.path.join(os.path.dirname(HERE), "include"), "-I",
                    os.path.join(PKG, "csrc"), os.path.join(HERE, "cpp", "general_layout_unit.cpp"), "-L", PKG,
                    "-lmxd_amd", "-Wl,-rpath," + PKG, "-o", exe], check=True, capture_output=True, timeout=300)

    def call(launches):
        text = []
        for f32, entries in launches:
            text.append("%d %d" % (int(f32), len(entries)))
            for e in entries:
                text.append(" ".join(str(int(e[k])) for k in (
                    "src_w", "src_h", "channels", "resize_w", "resize_h", "crop_x", "crop_y", "crop_w", "crop_h", "flip"))
                    + " %d %d %d %d %d %d" % (e["src"] - 4096, e["src_stride"], e["dst"] - 4096, e["dst_stride"],
                                              e.get("rgba_weighted", 0), e.get("filter", 0)))
        r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        lines = r.stdout.splitlines()
        assert lines[-1] == "ok"
        out = []
        for line in lines[:-1]:
            kind, rest = line.split(" ", 1)
            if kind == "launch" and not rest.startswith("rc=0"):
                rc, msg = rest.split(" ", 1)
                out.append((int(rc[3:]), msg[len("error="):]))
            else:
                f = {k: int(v) for k, v in (x.split("=") for x in rest.split())}
                if kind == "launch":
                    out.append((f, []))
                else:
                    assert kind == "image"
                    out[-1][1].append(f)
        assert len(out) == len(launches)
        return out

    return call


def model(entries):
    """What general_shapes restates of a launch: (vec, launch_cfg, tilings)."""
    vec = 16 if all((e["src"] | e["src_stride"]) % 16 == 0 for e in entries) else 1
    ts = [G.tiling((e["src_h"], e["src_w"], e["channels"]),
                   tuple(e[k] for k in ("resize_w", "resize_h", "crop_x", "crop_y", "crop_w", "crop_h", "flip")), vec,
                   e.get("filter", 0)) for e in entries]
    return vec, G.launch_cfg(ts), ts


def assert_same(got, entries, f32, tag):
    launch, images = got
    vec, cfg, ts = model(entries)
    assert (launch["vec"], launch["channels"], launch["f32"], launch["nimgs"]) == (
        vec, entries[0]["channels"], int(f32), len(entries)), (tag, launch)
    assert launch["alpha"] == int(entries[0]["channels"] == 4 and entries[0].get("rgba_weighted", 0)), (tag, launch)
    assert (launch["ntiles"], launch["smem"]) == (cfg["ntiles"], cfg["smem"]), (tag, launch, cfg)
    assert launch["max_vw"] == max(t["vw"] for t in ts), (tag, launch)  # (the planner's own figure)
    for k, (im, t) in enumerate(zip(images, ts)):
        assert im["index"] == k, (tag, k, im)
        assert [im[f] for f in ("nstrips", "tx", "ty", "group", "vw", "tile_begin", "xwidth", "ywidth")] == [
            t["nstrips"], t["tx"], t["ty"], t["group"], t["vw"], cfg["tile_begin"][k], t["xw"], t["yw"]], (tag, k, im, t)
    return launch, ts


def test_the_table_covers_every_instantiation():
    keys = G.instantiations()
    assert len(keys) == 20
    short = {(v, c, a) for v, c, _, a in keys}
    assert keys == {(v, c, f, a) for v, c, a in short for f in (False, True)}
    assert set(G.SHAPES) == short, ("without a shape", sorted(short - set(G.SHAPES)),
                                    "not in resample.hip", sorted(set(G.SHAPES) - short))


def test_a_new_instantiation_is_noticed(tmp_path):
    text = open(G.RESAMPLE_HIP).read()
    anchor = "    case 9: return launch_t<VEC, 4, true>(cfg, i, vw, xs, ys, xo, yo, s);\n"
    assert anchor in text
    hip = tmp_path / "resample.hip"
    hip.write_text(text.replace(anchor, anchor + "    case 10: return launch_t<VEC, 5, false>(cfg, i, vw, xs, ys, xo, yo, s);\n"))
    assert G.instantiations(str(hip)) - G.instantiations() == {(16, 5, False, False), (1, 5, False, False)}
    anchor = "  if (cfg.vec == 1) return launch_v<1>(cfg, imgs, vw, xs, ys, x_off, y_off, s);\n"
    assert anchor in text
    hip.write_text(text.replace(anchor, anchor + anchor.replace("== 1", "== 4").replace("<1>", "<4>")))
    assert {k[0] for k in G.instantiations(str(hip)) - G.instantiations()} == {4}


@needs_hipcc
@pytest.mark.parametrize("key", KEYS, ids=G.key_id)
def test_every_shape_has_its_tiling(key, unit):
    vec, c, alpha = key
    launches, tags = [], []
    for layout in G.layouts_of(vec):
        for f32 in (False, True):
            entries = []
            for sw, sh, cw, ch in G.SHAPES[key]:
                for g in W.windows(cw, ch):
                    assert G.is_general((sh, sw, c), g, layout, f32)
                    entries.append(G.entry((sh, sw, c), g, layout, f32, rgba_weighted=int(alpha)))
            launches.append((f32, entries))
            tags.append((key, layout, f32))
    for got, (f32, entries), tag in zip(unit(launches), launches, tags):
        launch, ts = assert_same(got, entries, f32, tag)
        assert launch["vec"] == vec and launch["alpha"] == int(alpha)
        one, two = ts[0:2], ts[4:6]  # the whole frames, plain and mirrored
        (_, _, _, ch0), (_, _, _, ch1) = G.SHAPES[key]
        assert ch0 <= 20 and ch1 % 32 not in (0,) and ch1 > 32
        for t in one:
            assert t["nstrips"] == 1 and t["nbands"] == 1 and t["ntiles"] == 1, (tag, t)
        for t in two:
            assert t["nstrips"] >= 2 and t["last_tx"] < t["tx"], (tag, t)
            assert t["nbands"] >= 2 and 0 < t["last_ty"] < t["ty"] == 32 and t["group"] < t["ty"], (tag, t)
    for which in (0, 1):
        assert G.fits(key, which, G.SHAPES[key][which]), (key, which)


def extra_launches(name):
    """[(f32, entries)] of every launch tests/test_gpu_general_shapes.py makes of the case (one destination layout)."""
    case = G.EXTRA[name]
    weighted = case.get("weighted") or [0] * len(case["images"])
    out = []
    for layouts in case["layouts"]:
        layouts = [layouts] * len(case["images"]) if isinstance(layouts, str) else list(layouts)
        for f32 in (False, True):
            entries = []
            for ((sw, sh), g), lay, a in zip(case["images"], layouts, weighted):
                assert G.is_general((sh, sw, case["c"]), tuple(g), lay, f32, case.get("filter", 0)), (name, g)
                entries.append(G.entry((sh, sw, case["c"]), tuple(g), lay, f32, case.get("filter", 0), a))
            out.append((f32, entries, layouts))
    return out


def sub_batches(entries):
    """split_batch's order for one channel count: weighted RGBA first."""
    if len({e["rgba_weighted"] for e in entries}) == 1:
        return [entries]
    return [[e for e in entries if e["rgba_weighted"]], [e for e in entries if not e["rgba_weighted"]]]


@needs_hipcc
@pytest.mark.parametrize("name", sorted(G.EXTRA))
def test_every_named_launch_has_its_property(name, unit):
    case = G.EXTRA[name]
    props = case["props"]
    launches = [(f32, sub, layouts) for f32, entries, layouts in extra_launches(name) for sub in sub_batches(entries)]
    results = unit([(f32, entries) for f32, entries, _ in launches])
    constants = G.constants()
    for got, (f32, entries, layouts) in zip(results, launches):
        if case.get("refused"):
            assert got == (capi.MXD_ERR_UNSUPPORTED, "mxd: tile does not fit in LDS"), (name, got)
            _, cfg, _ = model(entries)
            assert cfg["smem"] > constants["kLdsMax"], (name, cfg)
            continue
        launch, ts = assert_same(got, entries, f32, (name, layouts[0], f32))
        assert launch["smem"] <= constants["kLdsMax"]
        if "vec" in props and len(set(layouts)) == 1:
            assert launch["vec"] == props["vec"][layouts[0]], (name, layouts[0], launch)
        if len(set(layouts)) > 1:  # one unaligned image: the whole launch is VEC = 1
            assert sorted(G.vec_of(e["src_w"], e["channels"], lay) for e, lay in zip(entries, layouts))[:2] == [1, 16]
            assert launch["vec"] == 1, (name, layouts, launch)
        if "ntiles" in props:
            assert launch["ntiles"] == props["ntiles"], (name, launch)
        if "smem" in props:
            lo, hi = props["smem"]
            assert lo < launch["smem"] <= hi, (name, launch["smem"])
        if "group" in props:
            assert all(t["group"] == props["group"] for t in ts), (name, ts)
        if "by_budget" in props:  # kLdsBudget / (vw * 4), before the clamp to 1
            assert all(t["by_budget"] == props["by_budget"] and t["tx"] == 4 for t in ts), (name, ts)
        if "strips" in props:
            assert all(t["nstrips"] >= props["strips"] for t in ts[:2]), (name, ts)  # (the whole frame and its mirror image)
        if "all_differ" in props and len(set(layouts)) == 1:
            for f in props["all_differ"]:
                assert len({t[f] for t in ts}) == len(ts), (name, f, [t[f] for t in ts])
        if "ytaps_mod4" in props:
            counts = set()
            for e in entries:
                _, cnt, _ = capi.axis_taps(e["src_h"], e["resize_h"])
                counts |= set(cnt[e["crop_y"]:e["crop_y"] + e["crop_h"]].tolist())
            assert {n % 4 for n in counts} == {0, 1, 2, 3} and set(props["ytaps_mod4"]) <= counts, (name, sorted(counts))
        if "row_end" in props:  # elements of the last quad of a strip's rows
            ends = {(t["last_tx"] * e["channels"]) % 4 for t, e in zip(ts, entries)}
            assert ends == set(props["row_end"]), (name, ends)
        if "xtaps_over" in props:
            assert max(t["xw"] for t in ts) > props["xtaps_over"] or max(t["yw"] for t in ts) > props["xtaps_over"]


def test_the_finder_reproduces_the_table():
    for key in KEYS:
        for which in (0, 1):
            assert G.find(key, which) == G.SHAPES[key][which], (key, which)


def _frames():
    for key in KEYS:
        for k, (sw, sh, cw, ch) in enumerate(G.SHAPES[key]):
            for g in W.windows(cw, ch):
                yield key, k, (sw, sh), g, key[1], int(key[2])
    for name, case in sorted(G.EXTRA.items()):
        if case.get("filter") or case.get("refused"):
            continue
        weighted = case.get("weighted") or [0] * len(case["images"])
        seen = {}
        for (src, g), a in zip(case["images"], weighted):
            seen.setdefault((src, a), len(seen))
            yield name, seen[src, a], src, tuple(g), case["c"], a and case.get("plane", "holes")


def test_the_references_agree_within_the_gate():
    """No frame of SHAPES reaches 64 rows (they have 20 and 37), so the frames the
    gate covers are the few named launches' of 64 x 64 and more: one- and
    two-channel ones, none weighted and none of four channels."""
    checked = 0
    for key, k, (sw, sh), g, c, weighted in _frames():
        if g[4] < 64 or g[5] < 64:
            continue
        img = synth(sh, sw, c, G.seed_of(key, k))
        if weighted:
            img = G.ALPHA_PLANES[weighted](img)
            got = O.resize_crop_vfirst_rgba(img, g)
        else:
            got = O.resize_crop_vfirst(img, g)
        m, frac = compare(got, oracle_out(img, g, rgba_weighted=bool(weighted)))
        assert m <= 1 and frac < MAX_FRAC, (key, k, g, m, frac)
        checked += 1
    assert checked >= 3


DEEP = sorted(n for n, case in G.EXTRA.items() if case.get("deep"))


@pytest.mark.parametrize("name", DEEP)
def test_deep_ratio_tables_are_the_oracles(name):
    """first / count / weights of mxd_axis_taps against the oracle's restated
    stbir triangle filter, bit for bit, at ratios of 100 : 1 to 2400 : 1."""
    assert len(DEEP) >= 5
    axes = set()
    for (sw, sh), g in G.EXTRA[name]["images"]:
        axes |= {(sw, g[0]), (sh, g[1])}
    assert max(i / o for i, o in axes) >= 100
    for i, o in sorted(axes):
        n0, n1, w = O.axis_coeffs(i, o)
        first, cnt, pw = capi.axis_taps(i, o)
        assert np.array_equal(first, n0) and np.array_equal(cnt, n1 - n0 + 1), (name, i, o)
        for j in range(o):
            n = cnt[j]
            assert np.array_equal(w[j, :n].view(np.uint32), pw[j, :n].view(np.uint32)), (name, i, o, j)
            assert not pw[j, n:].any()


def test_the_weighted_filter_reference_is_the_oracles_on_triangle_tables():
    """filter_ref.vfirst's alpha-weighted form over the product's triangle tables
    against the oracle's own orc_resize_crop_vfirst_rgba, bit for bit: the
    weighted cubic case's reference differs from it by the tables alone."""
    import filter_ref

    for plane in sorted(G.ALPHA_PLANES):
        img = G.ALPHA_PLANES[plane](synth(75, 385, 4, 11))
        for g in W.windows(129, 37):
            assert np.array_equal(filter_ref.vfirst(img, g, "triangle", True), O.resize_crop_vfirst_rgba(img, g)), (plane, g)


NEGATIVE = sorted(n for n, case in G.EXTRA.items() if case.get("negative_alpha"))


@pytest.mark.parametrize("name", NEGATIVE)
def test_negative_alpha_cases_have_negative_alpha(name):
    """Whole output pixels whose filtered alpha is clearly negative (below -1 / 255),
    in the whole frame and its mirror image; the reference keeps their
    premultiplied colours (negative too: bytes of 0) where dividing by the alpha
    would give the colours back."""
    import filter_ref

    assert NEGATIVE
    case = G.EXTRA[name]
    for k, ((sw, sh), g) in enumerate(case["images"][:2]):
        g = tuple(g)
        img = G.ALPHA_PLANES[case["plane"]](synth(sh, sw, 4, G.seed_of(name, 0)))
        neg = G.filtered_alpha(img, g, case["filter"]) < -1.0 / 255
        assert neg.sum() >= 16, (name, g, int(neg.sum()))
        want = filter_ref.vfirst(img, g, case["filter"], True)
        assert (want[neg][:, 3] == 0).all(), (name, g)
        assert (want[neg][:, :3] <= 1).all(), (name, g)
