"""CPU: the seeded-noise generator's numpy restatement (tests/philox_ref.py) against the Random123 known answers and its own
identities, and the host side of the feature: the pass options, the noise-mode constants and the NbGeneratorInputs binding against
include/neube_hip.h.  The GPU tests (tests/test_hip_noise_seeded.py, ...) compare the kernel with this restatement."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import philox_ref as pr
from brushstroke_engine_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    got = pr.philox4x32_10(counter, key)
    assert tuple(int(v) for v in got) == want
    # ... and as one element of an array call (the form seeded_noise uses)
    arr = pr.philox4x32_10(tuple(np.array([1, c, 2], dtype=np.uint64) for c in counter), key)
    assert tuple(int(v[1]) for v in arr) == want


def test_uniform_mapping_and_box_muller():
    a = np.array([0, 0xffffffff, 0xff, 0x100], dtype=np.uint64)
    b = np.array([0, 0xffffffff, 0x40000000, 0x80000000], dtype=np.uint64)
    ze, zo, r = pr.normal_pair(a, b)
    np.testing.assert_allclose(r, np.sqrt(-2 * np.log([2.0 ** -24, 1.0, 2.0 ** -24, 2.0 ** -23])), rtol=1e-15)
    assert r[1] == 0 and ze[1] == 0 and zo[1] == 0                       # u1 = 1
    assert ze[0] == r[0] and zo[0] == 0                                  # angle 0
    assert ze[2] == 0 and zo[2] == r[2]                                  # angle pi / 2, reduced exactly
    assert ze[3] == -r[3] and zo[3] == 0                                 # angle pi
    u2 = (0xdeadbeef >> 8) * 2.0 ** -24
    ze, zo, r = pr.normal_pair(np.array([0x12345678], dtype=np.uint64), np.array([0xdeadbeef], dtype=np.uint64))
    np.testing.assert_allclose([ze[0], zo[0]], [r[0] * math.cos(2 * math.pi * u2), r[0] * math.sin(2 * math.pi * u2)], rtol=1e-14)


def test_reference_batch_split_identity_and_independence():
    """Sample k at offset o is sample 0 at offset o + k, across the 32-bit carry and the 64-bit wrap; seed, layer and sample select
    independent streams; a pixel depends on its quad alone (a larger image starts with the smaller one's values)."""
    for o, k in ((7, 3), (2 ** 32 - 2, 3), (2 ** 64 - 1, 1), (2 ** 64 - 1, 0)):
        np.testing.assert_array_equal(pr.seeded_noise(5, o, 2, k, 8)[0], pr.seeded_noise(5, (o + k) % 2 ** 64, 2, 0, 8)[0])
    base = pr.seeded_noise(5, 7, 2, 0, 8)[0]
    for other in (pr.seeded_noise(6, 7, 2, 0, 8), pr.seeded_noise(5 + 2 ** 32, 7, 2, 0, 8), pr.seeded_noise(5, 8, 2, 0, 8),
                  pr.seeded_noise(5, 7 + 2 ** 32, 2, 0, 8), pr.seeded_noise(5, 7, 3, 0, 8)):
        assert (other[0] != base).mean() > 0.9
    np.testing.assert_array_equal(pr.seeded_noise(5, 7, 2, 0, 5)[0].reshape(-1)[:24], base.reshape(-1)[:24])
    z, r = pr.seeded_noise(5, 7, 2, 0, 5)
    assert z.shape == r.shape == (5, 5) and (np.abs(z) <= r).all()


@pytest.mark.parametrize("seed", pr.STAT_SEEDS)
def test_reference_statistics_at_the_gpu_tests_seeds(seed):
    z = np.stack([pr.seeded_noise(seed, 0, 0, k, pr.STAT_RES)[0] for k in range(pr.STAT_N)])
    assert z.size == 16384
    pr.check_statistics(z, f"seed {seed}")


def test_pass_options_accept_seeded():
    from brushstroke_engine_amd.networks import _PassOptions
    o = _PassOptions.from_kwargs({"noise_mode": "seeded", "_noise_seed": (2 ** 64 + 3, -1)})
    assert o.noise_mode == "seeded" and o.noise_seed == (3, 2 ** 64 - 1) and o.noise_state is None
    state = object()
    o = _PassOptions.from_kwargs({"noise_mode": "seeded", "_noise_state": state})
    assert o.noise_state is state and o.noise_seed is None
    with pytest.raises(ValueError, match="exactly one"):
        _PassOptions.from_kwargs({"noise_mode": "seeded"})
    with pytest.raises(ValueError, match="exactly one"):
        _PassOptions.from_kwargs({"noise_mode": "seeded", "_noise_seed": (1, 0), "_noise_state": state})
    for mode in ("const", "random", "none"):
        with pytest.raises(ValueError, match="needs noise_mode 'seeded'"):
            _PassOptions.from_kwargs({"noise_mode": mode, "_noise_seed": (1, 0)})
        with pytest.raises(ValueError, match="needs noise_mode 'seeded'"):
            _PassOptions.from_kwargs({"noise_mode": mode, "_noise_state": state})
        assert _PassOptions.from_kwargs({"noise_mode": mode}).noise_mode == mode
    assert _PassOptions.from_kwargs({}).noise_mode == "random"                  # the reference's default stays


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "neube_hip.h")).read(), flags=re.S)


def test_noise_mode_constants_match_header():
    defines = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define NB_NOISE_([A-Z]+)\s+(-?\d+)", _header())}
    defines.pop("in", None)                                                       # NB_NOISE_IN_KERNEL is no mode
    assert defines == _lib.NB_NOISE_MODES
    assert _lib.NB_NOISE_MODES["seeded"] == 3 and _lib.NB_NOISE_MODES["random"] == 2


def test_generator_inputs_binding_has_the_headers_fields():
    body = re.search(r"typedef struct NbGeneratorInputs \{(.*?)\} NbGeneratorInputs;", _header(), flags=re.S).group(1)
    names, sizes = [], []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        pointer = "*" in decl
        ctype = re.match(r"(?:const\s+)?(\w+)", decl).group(1)
        for part in decl.split(","):
            m = re.search(r"(\w+)\s*(?:\[(\d+)\])?$", part.strip())
            names.append(m.group(1))
            width = 8 if pointer or ctype in ("uint64_t", "int64_t") else 4
            sizes.append(width * int(m.group(2) or 1))
    fields = _lib.NbGeneratorInputs._fields_
    assert [f[0] for f in fields] == names
    assert [ctypes.sizeof(f[1]) for f in fields] == sizes
    assert names[-3:] == ["noise_seed", "noise_offset", "noise_state"]
    assert _lib.NbGeneratorInputs.noise_seed.offset % 8 == 0
    assert ctypes.sizeof(_lib.NbGeneratorInputs) == _lib.NbGeneratorInputs.noise_state.offset + 8
    assert "nb_noise_seeded_f32" in _lib.PROTOTYPES and len(_lib.PROTOTYPES["nb_noise_seeded_f32"][1]) == 9
