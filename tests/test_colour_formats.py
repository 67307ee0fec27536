"""CPU tier of the colour-frame feature: the pixel-format constants of the header and of the Python module agree, and the numpy conversion the GPU tests
are held to (colour_util.to_gray) is the conversion the examples have always run on the host (examples/image_io.h: to_gray), on every (R, G, B)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import lvt_amd
import colour_util as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_enum_equals_the_python_constants():
    txt = open(os.path.join(ROOT, "include", "lvt_amd_ext.h")).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"LVT_AMD_PIX_(\w+)\s*=\s*(\d+)", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    assert enum == {"GRAY8": 0, "BGR8": 1, "RGB8": 2, "BGRA8": 3, "RGBA8": 4}, enum
    for name, value in enum.items():
        assert getattr(lvt_amd, "PIX_" + name) == value == getattr(CU, name)
    assert lvt_amd.PIX_BPP == CU.BPP
    for s in ("lvt_amd_set_pixel_format", "lvt_amd_batch_set_pixel_format", "lvt_amd_get_pixel_format"):
        assert s in lvt_amd.ABI_SYMBOLS


def test_known_answers():
    for (r, g, b), want in CU.KNOWN_ANSWERS:
        assert int(CU.gray_of_rgb(r, g, b)) == want, (r, g, b)
    lv = np.arange(256)
    assert np.array_equal(CU.gray_of_rgb(lv, lv, lv), lv.astype(np.uint8))   # (4899 + 9617 + 1868 = 16384: R = G = B = g gives g, for every g)
    # ... and through the packed formats: the channel order is the format's, the alpha byte is not used
    px = {CU.RGB8: [255, 0, 0], CU.BGR8: [0, 0, 255], CU.RGBA8: [255, 0, 0, 77], CU.BGRA8: [0, 0, 255, 201]}
    for fmt, p in px.items():
        assert int(CU.to_gray(np.array([[p]], np.uint8), fmt)[0, 0]) == 76, CU.NAMES[fmt]


def test_colourised_frames_convert_alike_in_every_format():
    """the colour inputs of the GPU tests: one draw per (world, frame, eye), packed per format -- every format converts to the same gray image, and a swapped
    channel order or a used alpha byte would change most of its pixels"""
    g = np.random.default_rng(3).integers(0, 256, size=(37, 53), dtype=np.uint8)
    ref = CU.to_gray(CU.colourise(g, CU.RGB8, 71, 2, 1), CU.RGB8)
    for fmt in CU.COLOUR_FORMATS:
        img = CU.colourise(g, fmt, 71, 2, 1)
        assert img.shape == (37, 53, CU.BPP[fmt])
        assert np.array_equal(CU.to_gray(img, fmt), ref), CU.NAMES[fmt]
    swapped = CU.to_gray(CU.colourise(g, CU.BGR8, 71, 2, 1), CU.RGB8)
    assert np.mean(swapped != ref) > 0.5
    r, gg, b, a = CU.colour_channels(g, 71, 2, 1)
    assert np.mean(CU.gray_of_rgb(gg, b, a) != ref) > 0.5          # (a 4-byte pixel read one byte late)
    assert not np.array_equal(CU.colourise(g, CU.RGB8, 71, 3, 1), CU.colourise(g, CU.RGB8, 71, 2, 1))


def test_numpy_conversion_equals_the_examples_to_gray(tmp_path):
    """all 2^24 (R, G, B) triples through examples/image_io.h: to_gray, compiled into a stand-alone program, against colour_util.gray_of_rgb"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no C++ compiler")
    src = tmp_path / "all_triples.cpp"
    src.write_text('#include "image_io.h"\n#include <cstdio>\n'
                   "int main() { std::vector<unsigned char> o(1u << 24); for (int i = 0; i < (1 << 24); i++) o[i] = lvt_io::to_gray(i >> 16, (i >> 8) & 255, i & 255);\n"
                   "  return std::fwrite(o.data(), 1, o.size(), stdout) == o.size() ? 0 : 1; }\n")
    exe = tmp_path / "all_triples"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "examples"), "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, timeout=120)
    assert out.returncode == 0 and len(out.stdout) == 1 << 24
    got = np.frombuffer(out.stdout, np.uint8)
    i = np.arange(1 << 24, dtype=np.int64)
    want = CU.gray_of_rgb(i >> 16, (i >> 8) & 255, i & 255)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} triples differ, first (R, G, B) = {(int(bad[0]) >> 16, (int(bad[0]) >> 8) & 255, int(bad[0]) & 255)}"


def test_u8_refuses_a_shape_that_is_not_the_formats():
    """lvt_amd._u8: a colour image on a gray handle (or the other way round, or the wrong number of channels) raises instead of being flattened"""
    gray, rgb, rgba = np.zeros((4, 6), np.uint8), np.zeros((4, 6, 3), np.uint8), np.zeros((4, 6, 4), np.uint8)
    assert lvt_amd._u8(gray).shape == (4, 6) and lvt_amd._u8(rgb, 3).shape == (4, 6, 3) and lvt_amd._u8(rgba, 4).shape == (4, 6, 4)
    assert lvt_amd._u8(rgb, 3) is rgb                                  # (a contiguous uint8 array is used as it is)
    for img, bpp in ((rgb, 1), (rgba, 1)):
        with pytest.raises(AssertionError):
            lvt_amd._u8(img, bpp)
    for img, bpp in ((gray, 3), (rgba, 3), (rgb, 4), (gray, 4)):
        with pytest.raises(ValueError):
            lvt_amd._u8(img, bpp)


def test_facade_takes_colour_views(tmp_path):
    """include/lvt_system.h: set_pixel_format, the colour constructor of lvt_image_view and the bytes-per-pixel checks of track / track_async compile
    (no OpenCV, no Eigen, warnings are errors) and link; with a GPU the program tracks one RGB8 pair and a gray view is then turned away"""
    cxx = shutil.which("g++")
    if not cxx or not os.path.exists(lvt_amd.LIB_PATH):
        pytest.skip("no g++, or the library has not been built")
    src = tmp_path / "colour_caller.cpp"
    src.write_text(r'''
#include "lvt_system.h"
#include <cstdio>
int main() {
    lvt_parameters params;
    params.fx = params.fy = 300.f; params.cx = 160.f; params.cy = 60.f; params.baseline = 0.5f;
    params.img_width = 320; params.img_height = 120;
    lvt_system *vo = lvt_system::create(params, lvt_system::eSensor_STEREO);
    if (!vo) { std::printf("no device\n"); return 0; }
    if (!vo->set_pixel_format(LVT_AMD_PIX_RGB8)) return 3;
    std::vector<unsigned char> rgb(320 * 120 * 3, 90), padded((320 * 3 + 7) * 120, 90), gray(320 * 120, 90);
    vo->track(lvt_image_view(rgb.data(), 120, 320, 3, 0), lvt_image_view(padded.data(), 120, 320, 3, 320 * 3 + 7));
    if (vo->last_error()[0]) { std::printf("%s\n", vo->last_error()); return 4; }
    if (vo->track_async(lvt_image_view(gray.data(), 120, 320), lvt_image_view(gray.data(), 120, 320))) return 5;   // a gray view on a colour system
    if (!vo->track_async(lvt_image_view(rgb.data(), 120, 320, 3, 0), lvt_image_view(rgb.data(), 120, 320, 3, 0))) return 6;
    vo->wait_pose();
    if (!vo->set_pixel_format(LVT_AMD_PIX_GRAY8)) return 7;
    if (!vo->track_async(lvt_image_view(gray.data(), 120, 320), lvt_image_view(gray.data(), 120, 320))) return 8;
    vo->wait_pose();
    if (vo->set_pixel_format(99) || !vo->last_error()[0]) return 2;   // refused with a reason: nothing changed
    if (!vo->track_async(lvt_image_view(gray.data(), 120, 320), lvt_image_view(gray.data(), 120, 320))) return 9;
    vo->wait_pose();
    lvt_system::destroy(vo);
    return 0;
}
''')
    exe = tmp_path / "colour_caller"
    libdir = os.path.dirname(lvt_amd.LIB_PATH)
    subprocess.check_call([cxx, "-std=c++11", "-Wall", "-Werror", "-DLVT_SYSTEM_NO_OPENCV", "-DLVT_SYSTEM_NO_EIGEN", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                           str(src), "-L", libdir, "-llvt_c", "-Wl,-rpath," + libdir])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
