"""run_wave_chain(sources=...): an extended, spatially incoherent source through the Wavecalc chain
on the MI355X. Row s of every field is, bit for bit, the single-source chain's with
points_source.npy = sources[:, s]; the intensities are the weighted sums of |u|^2 in the documented
numpy form. The 17 x 17 AKB file set is that of test_wave_chain_resume_every_mirror_stage."""
import os
import shutil

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

NAMES = ("M1", "M2", "M3", "M4", "Image", "Image2")


@pytest.fixture(scope="module")
def chain(gpu, tmp_path_factory):
    """The file set, three source points (the file's own, two offset by a few um in y and z), the
    extended-source run with its output directory, and the three single-source runs."""
    from akbraytracing_amd import wavedata as W
    root = tmp_path_factory.mktemp("wave_sources")
    folder = root / "set"
    f = golden("akb_raywave_65.npz")
    hits = f["pass2_hits"].reshape(4, 3, 65, 65)[:, :, ::4, ::4].reshape(4, 3, -1)
    det = f["detcenter"].reshape(3, 65, 65)[:, ::4, ::4].reshape(3, -1)
    det2 = f["detcenter2"].reshape(3, 65, 65)[:, ::4, ::4].reshape(3, -1)
    W.save_wave_data(str(folder), np.zeros((3, 1)), list(hits), 17, 17, det, det2, defocus_for_wave=1e-2)
    own = np.load(folder / "points_source.npy")
    P = np.stack([own, own + [0.0, 3e-6, -2e-6], own + [0.0, -4e-6, 5e-6]], axis=1)
    w = np.array([0.5, 0.3, 0.2])
    fields = W.run_wave_chain(str(folder), str(root / "ext"), resume_dir=None, sources=P, weights=w)
    singles = []
    for s in range(3):
        copy = root / f"single{s}"
        shutil.copytree(folder, copy)
        np.save(copy / "points_source.npy", P[:, s])
        singles.append(W.run_wave_chain(str(copy), None, resume_dir=None))
    return dict(folder=folder, root=root, P=P, w=w, fields=fields, singles=singles)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("name", NAMES)
def test_every_row_is_the_single_source_chain(chain, name):
    u = chain["fields"][name]
    assert u.dtype == np.complex128 and u.shape == (3,) + chain["singles"][0][name].shape
    for s in range(3):
        assert _same_bits(u[s], chain["singles"][s][name]), (name, s)
    # the offset points light the surfaces differently
    assert not np.array_equal(u[0], u[1]) and not np.array_equal(u[0], u[2])


def test_intensities_and_the_files_written(chain):
    fields, w = chain["fields"], chain["w"]
    assert sorted(fields) == sorted(NAMES + ("Image_intensity", "Image2_intensity"))
    out = chain["root"] / "ext"
    for name in ("Image", "Image2"):
        u = fields[name]
        want = (w[:, None] * (u.real**2 + u.imag**2)).sum(axis=0)
        got = fields[f"{name}_intensity"]
        assert got.dtype == np.float64 and _same_bits(got, want)
        assert _same_bits(np.load(out / f"intensity_{name}.npy"), want)
    assert sorted(p.name for p in out.iterdir()) == sorted(
        [f"complex_data_{n}.npz" for n in NAMES] + ["intensity_Image.npy", "intensity_Image2.npy"])
    for name in NAMES:
        with np.load(out / f"complex_data_{name}.npz") as z:
            assert _same_bits(z["data"], fields[name])


def test_default_weights_are_equal(chain):
    from akbraytracing_amd import wavedata as W
    fields = W.run_wave_chain(str(chain["folder"]), None, resume_dir=str(chain["root"] / "ext"), sources=chain["P"])
    u = fields["Image"]
    want = (np.full(3, 1.0 / 3)[:, None] * (u.real**2 + u.imag**2)).sum(axis=0)
    assert _same_bits(fields["Image_intensity"], want)


def test_resume_from_the_stacked_files(chain, tmp_path):
    from akbraytracing_amd import wavedata as W
    resumed = []
    again = W.run_wave_chain(str(chain["folder"]), str(tmp_path / "run2"), resume_dir=str(chain["root"] / "ext"),
                             resumed=resumed, sources=chain["P"], weights=chain["w"])
    assert resumed == ["M1", "M2", "M3", "M4"]
    for name in NAMES + ("Image_intensity", "Image2_intensity"):
        assert _same_bits(again[name], chain["fields"][name]), name
    assert sorted(p.name for p in (tmp_path / "run2").iterdir()) == [
        "complex_data_Image.npz", "complex_data_Image2.npz", "intensity_Image.npy", "intensity_Image2.npy"]


def test_resume_from_one_stage_propagates_the_rest(chain, tmp_path):
    from akbraytracing_amd import wavedata as W
    shutil.copy(chain["root"] / "ext" / "complex_data_M2.npz", tmp_path)
    resumed = []
    again = W.run_wave_chain(str(chain["folder"]), None, resume_dir=str(tmp_path), resumed=resumed,
                             sources=chain["P"], weights=chain["w"])
    assert resumed == ["M2"]
    for name in NAMES:
        assert _same_bits(again[name], chain["fields"][name]), name


def test_a_resume_file_of_another_shape_is_refused(chain, tmp_path):
    from akbraytracing_amd import wavedata as W
    n = chain["fields"]["M1"].shape[1]
    for bad in (np.zeros(n, complex), np.zeros((2, n), complex), np.zeros((3, n + 1), complex)):
        np.savez(tmp_path / "complex_data_M1.npz", data=bad)
        with pytest.raises(ValueError):
            W.run_wave_chain(str(chain["folder"]), None, resume_dir=str(tmp_path), sources=chain["P"])
