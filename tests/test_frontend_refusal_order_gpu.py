"""Which refusal wins when two arguments of an STFT entry point are wrong at once (csrc/frontend.hip).  The four forwards and the four backwards
check their arguments in different orders -- orcai_stft_db the frame count before the alignment, the others the alignment, the transform size, the
frame count and then the band table -- and a caller sees that order in the return code.  tests/golden/frontend_refusal_order.json holds the code of
every single fault and of every unordered pair of faults from different categories, recorded from the library before the launchers came to share
their helpers; the codes must stay what they were.

Every case is refused on the host before the first HIP call, so the table depends on no device: record() below fills it from placeholder addresses
(run this file as a script to print it), and the test repeats the calls with real device buffers behind sentinel guards and asserts that none of
them was written.  A fault is listed for an entry only where the entry's contract in include/orcai_hip.h refuses it: orcai_stft_db runs every
n_fft up to 4096, the linear energy and backward entries the powers of two from 32, the mel entries those from 128; the linear backwards take any
alignment.  The orcai_make_* compositions reset the workspace before they check and are left to the tests of their own."""

import itertools
import json
from pathlib import Path

import numpy as np
import pytest

import mel_ref as MR
import stft_ref as R
from orcai_amd import mel

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "frontend_refusal_order.json"
N_FFT, HOP, N = 512, 256, 4100  # the valid call of test_mel_gpu.test_refusals: 17 frames, the 40-band HTK table
T = R.num_frames(N, N_FFT, HOP)
K_CROP = 171
GUARD = 64 + 3
SENTINEL_BITS = 0x7FC12345
TOP_DB = 80.0

SIZES = ["n_samples", "n_fft", "hop", "n_frames"]
BANDS = ["band_lo", "band_hi", "band_off", "weights", "n_weights"]
ENTRIES = {
    "orcai_stft_db": SIZES + ["k_crop", "out", "workspace"],
    "orcai_stft_mel_db": SIZES + ["n_mels"] + BANDS + ["out", "workspace"],
    "orcai_stft_energy": SIZES + ["k_crop", "out"],
    "orcai_stft_mel_energy": SIZES + ["n_mels"] + BANDS + ["out"],
    "orcai_spectrogram_bwd": SIZES + ["k_crop", "gout", "stats", "top_db", "dpcm"],
    "orcai_stft_energy_bwd": SIZES + ["k_crop", "gout", "dpcm"],
    "orcai_mel_spectrogram_bwd": SIZES + ["n_mels"] + BANDS + ["gout", "stats", "top_db", "dpcm"],
    "orcai_stft_mel_energy_bwd": SIZES + ["n_mels"] + BANDS + ["gout", "dpcm"],
}
DEVICE_POINTERS = ("pcm", "weights", "out", "workspace", "gout", "stats", "dpcm")
# what the contract refuses of {64, 500, 384, 8192}
REFUSED_N_FFT = {"orcai_stft_db": (8192,), "orcai_stft_energy": (500, 384, 8192), "orcai_spectrogram_bwd": (500, 384, 8192),
                 "orcai_stft_energy_bwd": (500, 384, 8192)}


def band_tables():
    """The base table and its broken variants (host arrays; the caller keeps them alive): name -> {lo, hi, off}."""
    t = mel.band_table(MR.SR, N_FFT, *MR.MELS[N_FFT][1])
    n_mels, n_weights = t["lo"].size, t["weights"].size

    def with_(key, m, v):
        b = {k: t[k].copy() for k in ("lo", "hi", "off")}
        b[key][m] = v
        return b

    bad = {
        "band_lo < 0": with_("lo", 3, -1),
        "band_hi > 1 + n_fft / 2": with_("hi", 5, 258),
        "band_hi < band_lo": with_("hi", 2, int(t["lo"][2]) - 1),
        "band_off < 0": with_("off", 0, -4),
        "band_off past the weights": with_("off", n_mels - 1, n_weights),
    }
    # bands 0 and 2 share a bin (as test_mel_grad_gpu breaks its table): inside every range, refused by the backward's gather alone
    assert t["hi"][0] <= t["lo"][2]
    over = {k: t[k].copy() for k in ("lo", "hi", "off")}
    over["lo"][2] = t["hi"][0] - 1
    over["hi"][2] -= 1
    return t, bad, over


def faults(entry, tables):
    """[(category, label, {argument: new value})] for one entry; "+b" on a pointer means b bytes past it, None a null."""
    names = ENTRIES[entry]
    mel_entry, backward = "n_mels" in names, entry.endswith("_bwd")
    t, bad, over = tables
    out = []
    for p in ["pcm"] + [a for a in names if a in DEVICE_POINTERS]:
        out.append((p, f"null {p}", {p: None}))
    if not backward:
        out += [(p, f"misaligned {p}", {p: "+4"}) for p in ("pcm", "out") + (("weights",) if mel_entry else ())]
    elif mel_entry:
        out += [(p, f"misaligned {p}", {p: "+4"}) for p in ("pcm", "weights")]
        out += [(p, f"misaligned {p}", {p: "+2"}) for p in ("gout", "stats", "dpcm") if p in names]
    out += [("n_samples", "n_samples 0", {"n_samples": 0}), ("hop", "hop 0", {"hop": 0}), ("n_frames", "n_frames + 1", {"n_frames": T + 1}),
            ("n_frames", "n_frames - 1", {"n_frames": T - 1})]
    if mel_entry:
        out += [("n_mels", "n_mels 7", {"n_mels": 7}), ("n_mels", "n_mels 257", {"n_mels": 257}), ("n_weights", "n_weights 0", {"n_weights": 0}),
                ("n_weights", "n_weights 65536", {"n_weights": 65536})]
        out += [("band table", f"null {a}", {a: None}) for a in ("band_lo", "band_hi", "band_off")]
        table = lambda b: {"band_lo": b["lo"].ctypes.data, "band_hi": b["hi"].ctypes.data, "band_off": b["off"].ctypes.data}  # noqa: E731
        out += [("band table", what, table(b)) for what, b in bad.items()]
        if backward:
            out.append(("band table", "bands 0 and 2 overlap", table(over)))
    else:
        out += [("k_crop", "k_crop 0", {"k_crop": 0}), ("k_crop", "k_crop 258", {"k_crop": 258})]
    out += [("n_fft", f"n_fft {nf}", {"n_fft": nf}) for nf in REFUSED_N_FFT.get(entry, (64, 500, 384, 8192))]
    return out


def cases(entry, tables, device):
    """[(label, argument list)]: every single fault, then every unordered pair of faults from different categories.  device: name -> address of
    pcm, weights, out, workspace, gout, stats, dpcm (16-byte aligned) and the stream."""
    t = tables[0]
    base = dict(device, n_samples=N, n_fft=N_FFT, hop=HOP, n_frames=T, k_crop=K_CROP, n_mels=t["lo"].size, band_lo=t["lo"].ctypes.data,
                band_hi=t["hi"].ctypes.data, band_off=t["off"].ctypes.data, n_weights=t["weights"].size, top_db=TOP_DB)
    fs = faults(entry, tables)
    combos = [(f,) for f in fs] + [(f, g) for f, g in itertools.combinations(fs, 2) if f[0] != g[0]]
    out = []
    for combo in combos:
        a = dict(base)
        for _, _, change in combo:
            for k, v in change.items():
                a[k] = base[k] + int(v) if isinstance(v, str) else v
        out.append((" & ".join(f[1] for f in combo), [a[k] for k in ["pcm"] + ENTRIES[entry] + ["stream"]]))
    assert len({label for label, _ in out}) == len(out)
    return out


def record(lib, device):
    """{entry: {case: return code}} -- with placeholder addresses on a machine without a GPU, nothing here gets as far as a HIP call."""
    tables = band_tables()
    return {e: {label: getattr(lib, e)(*args) for label, args in cases(e, tables, device)} for e in ENTRIES}


PLACEHOLDERS = dict({p: 0x7F0000000000 + 0x100000 * i for i, p in enumerate(DEVICE_POINTERS, 1)}, stream=None)



@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_table_covers_every_entry_and_holds_refusals_only(golden):
    tables = band_tables()
    assert sorted(golden) == sorted(ENTRIES)
    for e in ENTRIES:
        labels = [label for label, _ in cases(e, tables, PLACEHOLDERS)]
        assert sorted(golden[e]) == sorted(labels), e
        assert set(golden[e].values()) <= {R.E_BADARG, R.E_UNSUPPORTED}, e


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_refusal_codes_are_the_recorded_ones_and_nothing_is_written(entry, golden):
    from orcai_amd import _native as N_

    lib = N_.lib()
    tables = band_tables()
    k_max = 258  # the widest row a case asks for (k_crop 258, n_mels 257); one frame more than the base call

    def buffer(count):
        return torch.full((count + GUARD,), SENTINEL_BITS, dtype=torch.int32, device="cuda")

    ws = torch.zeros(lib.orcai_frontend_workspace_bytes(), dtype=torch.uint8, device="cuda")
    assert lib.orcai_frontend_reset(ws.data_ptr(), N_.stream_ptr()) == 0
    torch.cuda.synchronize()
    ws_before = ws.clone()
    pcm = torch.tensor(MR.make_input("noise", N, N_FFT, HOP), device="cuda")
    weights = torch.tensor(tables[0]["weights"], device="cuda")
    gout = torch.zeros(((T + 1) * k_max,), device="cuda")
    stats = torch.tensor([1.0, 0.0, -60.0, -5.0, -60.0, -5.0, 0.0, 0.0], device="cuda")
    written = {"out": buffer((T + 1) * k_max), "dpcm": buffer(N + HOP)}
    device = dict(pcm=pcm.data_ptr(), weights=weights.data_ptr(), workspace=ws.data_ptr(), gout=gout.data_ptr(), stats=stats.data_ptr(),
                  stream=N_.stream_ptr(), **{k: b.data_ptr() for k, b in written.items()})
    assert all(v % 16 == 0 for k, v in device.items() if k != "stream")
    fn = getattr(lib, entry)
    got = {label: fn(*args) for label, args in cases(entry, tables, device)}
    torch.cuda.synchronize()
    wrong = {label: (code, golden[entry][label]) for label, code in got.items() if code != golden[entry][label]}
    assert not wrong, (entry, wrong)
    for name, b in written.items():
        assert bool((b == SENTINEL_BITS).all().item()), f"a refused {entry} wrote to {name}"
    assert torch.equal(ws, ws_before), f"a refused {entry} changed the workspace"


if __name__ == "__main__":  # prints the golden file's content
    from orcai_amd import _native as N_

    print(json.dumps(record(N_.lib(), PLACEHOLDERS), indent=0, sort_keys=True))
