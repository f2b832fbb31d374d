"""bench.py's pieces outside the timed steps that need no GPU: the kept corpus
(a kept copy is the bytes a fresh generation gives), --dump-outputs' files,
and the options of a plain / --full run."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_kept_corpus_is_the_generated_one(tmp_path):
    import bench
    d = str(tmp_path / "cache")
    fresh = bench.make_corpus("c4", 1 << 20, 0x5EED)
    first = bench.cached_corpus("c4", 1, 0x5EED, cache_dir=d)
    assert first[0] == fresh[0] and first[1] == fresh[1]
    stem = os.path.join(d, bench.corpus_key("c4", 1, 0x5EED))
    assert os.path.exists(stem + ".zst") and not os.path.exists(stem + ".src")
    assert not [n for n in os.listdir(d) if n.endswith(".tmp")]
    kept = bench.cached_corpus("c4", 1, 0x5EED, cache_dir=d)
    assert kept[0] == fresh[0] and kept[1] is None and kept[3] == 0.0
    # the source is wanted and was not kept: generated again, and kept where asked
    again = bench.cached_corpus("c4", 1, 0x5EED, cache_dir=d, need_src=True, keep_src=True)
    assert again[0] == fresh[0] and again[1] == fresh[1]
    both = bench.cached_corpus("c4", 1, 0x5EED, cache_dir=d, need_src=True)
    assert both[0] == fresh[0] and both[1] == fresh[1] and both[3] == 0.0
    # another seed, size or workload is another file
    keys = {bench.corpus_key("c4", 1, 0x5EED), bench.corpus_key("c4", 1, 0x5EEE), bench.corpus_key("c4", 2, 0x5EED),
            bench.corpus_key("c3", 1, 0x5EED), bench.corpus_key("c5", 1, 0x5EED, level=1),
            bench.corpus_key("c5", 1, 0x5EED, level=9)}
    assert len(keys) == 6


def test_dump_outputs_files(tmp_path):
    import bench
    total = (3 << 20) + 12345                      # three whole MiB chunks and a short one
    buf = torch.from_numpy(np.random.default_rng(7).integers(0, 256, size=total + 64, dtype=np.uint8))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), buf, total, 0)
    a = {n: np.load(tmp_path / "a" / n) for n in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["decoded_chunk_sums.npy", "decoded_len.npy", "decoded_sample.npy"]
    for n, v in a.items():
        assert v.dtype in (np.float32, np.float64)
        assert np.array_equal(v, np.load(tmp_path / "b" / n)), n      # the same positions every run
    assert a["decoded_len.npy"].tolist() == [0.0, float(total)]
    out = buf.numpy()[:total].astype(np.int64)
    want = [out[k:k + (1 << 20)].sum() for k in range(0, total, 1 << 20)]
    assert a["decoded_chunk_sums.npy"].tolist() == [float(w) for w in want]
    s = a["decoded_sample.npy"]
    assert s.shape == (total,) and s.min() >= 0 and s.max() <= 255
    # one changed byte shows in the sums
    buf2 = buf.clone()
    buf2[(2 << 20) + 5] ^= 0x40
    bench.dump_outputs(str(tmp_path / "c"), buf2, total, 0)
    c = np.load(tmp_path / "c" / "decoded_chunk_sums.npy")
    assert (c != a["decoded_chunk_sums.npy"]).tolist() == [False, False, True, False]


def test_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in out.stdout
