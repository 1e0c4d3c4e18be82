"""orcai_amd/pcen.py without a GPU: the parameter's validation, the float64 specification pcen_ref and the algebra of orcai_pcen's three-launch scan."""

import numpy as np
import pytest

from orcai_amd import mel, pcen

SP = {"sampling_rate": 48000, "nfft": 512, "n_overlap": 256, "freq_range": [0, 16000], "quantiles": [0.01, 0.999]}


def sp(**kw):
    return {**SP, **kw}


# ------------------------------------------------------------------------------------------------ pcen_config
def test_defaults_are_filled_in():
    cfg = pcen.pcen_config(sp(pcen={}))
    assert cfg == {"time_constant": 0.4, "gain": 0.98, "bias": 2.0, "power": 0.5, "eps": 1e-6, "scale": 2147483648.0}
    assert all(type(v) is float for v in cfg.values())
    cfg = pcen.pcen_config(sp(pcen={"time_constant": 1, "bias": 0, "gain": 0, "power": 1}))
    assert (cfg["time_constant"], cfg["bias"], cfg["gain"], cfg["power"]) == (1.0, 0.0, 0.0, 1.0) and cfg["eps"] == 1e-6


def test_null_and_absent_give_none():
    assert pcen.pcen_config(SP) is None
    assert pcen.pcen_config(sp(pcen=None)) is None
    assert pcen.pcen_config(sp(nfft=500)) is None  # nothing of the dB front end's is refused here


@pytest.mark.parametrize("key,bad", [("time_constant", 0), ("time_constant", -1.0), ("gain", -0.1), ("gain", 1.5), ("bias", -1e-9), ("power", 0), ("power", 1.01),
                                     ("eps", 0), ("scale", 0), ("scale", -2.0), ("gain", "0.5"), ("bias", True), ("eps", float("nan")), ("scale", float("inf")),
                                     ("power", None)])
def test_every_refusal_names_its_key(key, bad):
    with pytest.raises(ValueError, match=rf"pcen\.{key}\b"):
        pcen.pcen_config(sp(pcen={key: bad}))


def test_unknown_key_and_non_dict():
    with pytest.raises(ValueError, match="'alpha'"):
        pcen.pcen_config(sp(pcen={"alpha": 0.98}))
    for bad in (True, 1, "on", [0.4]):
        with pytest.raises(ValueError, match="pcen = "):
            pcen.pcen_config(sp(pcen=bad))


@pytest.mark.parametrize("nfft", [500, 1000, 16, 8192, 511])
def test_nfft_that_is_no_power_of_two_is_not_implemented(nfft):
    with pytest.raises(NotImplementedError, match="nfft"):
        pcen.pcen_config(sp(nfft=nfft, pcen={}))
    for ok in (32, 128, 512, 4096):
        assert pcen.pcen_config(sp(nfft=ok, pcen={})) is not None


def test_works_together_with_mel():
    p = sp(mel={"n_mels": 64}, pcen={"time_constant": 0.1})
    assert mel.mel_config(p)["n_mels"] == 64
    assert pcen.pcen_config(p)["time_constant"] == 0.1
    with pytest.raises(ValueError, match="n_mels"):  # each key keeps its own refusals
        mel.mel_config(sp(mel={}, pcen={}))


# ------------------------------------------------------------------------------------------------ the smoother's coefficient
def test_b_against_its_closed_forms():
    a, b = pcen.smoother(1.0, 100.0, 100)  # t = 1 frame: b = (sqrt(5) - 1) / 2
    assert abs(b - (np.sqrt(5.0) - 1.0) / 2.0) <= 1e-15 and abs(a + b - 1.0) <= 1e-16
    for t in (1e3, 1e5):  # t large: sqrt(1 + 4 t^2) = 2 t + 1/(4 t) - 1/(64 t^3) + ..., so b = 1/t - 1/(2 t^2) + 1/(8 t^3) - 1/(128 t^5) + ...
        _, b = pcen.smoother(t, 1.0, 1)
        assert abs(b * t - 1.0) <= 0.6 / t
        # the subtraction sqrt(1 + 4 t^2) - 1 costs about 2^-53 * 2 t / (2 t^2) absolute: 1e-16 / t, rounded up tenfold
        assert abs(b - (1.0 / t - 0.5 / t**2 + 0.125 / t**3)) <= 1.0 / (128 * t**5) + 1e-15 / t
    a, b = pcen.smoother(0.4, 48000, 256)  # the default at 48 kHz, hop 256: t = 75 frames
    assert abs(b - (np.sqrt(1 + 4 * 75.0**2) - 1) / (2 * 75.0**2)) <= 1e-16 and 0.98 < a < 0.99


# ------------------------------------------------------------------------------------------------ pcen_ref
@pytest.mark.parametrize("params", [{}, {"bias": 0.0, "power": 1.0}, {"gain": 0.5, "eps": 1e-3, "scale": 1.0, "time_constant": 0.01}])
def test_constant_column_has_the_closed_form(params):
    cfg = pcen.pcen_config(sp(pcen=params))
    c = np.array([1e-7, 3e-4, 0.25])
    E = np.tile(c, (700, 1))
    out = pcen.pcen_ref(E, cfg, 48000, 256)
    S = cfg["scale"] * c  # M == S at every frame: a + b = 1
    want = (S * (cfg["eps"] + S) ** -cfg["gain"] + cfg["bias"]) ** cfg["power"] - cfg["bias"] ** cfg["power"]
    assert out.shape == E.shape
    assert np.abs(out - want[None, :]).max() <= 1e-12 * np.abs(want).max()
    assert (np.abs(out - want[None, :]) <= 1e-12 * np.maximum(np.abs(want), cfg["bias"] ** cfg["power"])[None, :]).all()


def test_all_zero_energy_is_exactly_zero():
    for params in ({}, {"bias": 0.0}, {"bias": 0.3, "power": 0.37}):
        cfg = pcen.pcen_config(sp(pcen=params))
        out = pcen.pcen_ref(np.zeros((300, 5)), cfg, 48000, 256)
        assert out.dtype == np.float64 and not out.any()


# ------------------------------------------------------------------------------------------------ the scan's algebra
def scan_f64(S: np.ndarray, a: float, b: float, chunk: int = pcen.CHUNK) -> np.ndarray:
    """M by orcai_pcen's three launches, restated in float64: per chunk the chain from zero (chunk 0 from M[0] = S[0]), the carries
    C[0] = P[0], C[j] = a^L_j C[j-1] + P[j] with L_j the chunk's own length, the chain again from C[j-1]."""
    T = S.shape[0]
    n_chunks = (T + chunk - 1) // chunk

    def chain(j, m, out=None):
        for t in range(j * chunk, min(T, (j + 1) * chunk)):
            m = S[t].copy() if t == 0 else a * m + b * S[t]
            if out is not None:
                out[t] = m
        return m

    P = [chain(j, np.zeros_like(S[0])) for j in range(n_chunks)]
    C = [P[0]]
    for j in range(1, n_chunks):
        length = min(T, (j + 1) * chunk) - j * chunk
        C.append(a**length * C[j - 1] + P[j])
    M = np.empty_like(S)
    for j in range(n_chunks):
        chain(j, C[j - 1] if j else None, M)
    return M


@pytest.mark.parametrize("T", [1, 255, 256, 257, 1030])
@pytest.mark.parametrize("time_constant", [0.4, 4.0])
def test_chunked_scan_equals_the_sequential_recurrence(T, time_constant):
    assert pcen.CHUNK == 256
    rng = np.random.default_rng(T)
    S = 10.0 ** rng.uniform(-9, 0, size=(T, 3)) * 2.0**31
    a, b = pcen.smoother(time_constant, 48000, 256)
    M = np.empty_like(S)
    M[0] = S[0]
    for t in range(1, T):
        M[t] = a * M[t - 1] + b * S[t]
    got = scan_f64(S, a, b)
    assert (got[0] == S[0]).all()
    assert np.abs(got - M).max() <= 1e-12 * np.abs(M).max()
    assert (np.abs(got - M) <= 1e-12 * M).all()
