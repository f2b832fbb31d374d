"""Regenerates the pinned dictionary fixture of tests/test_dict_gpu.py with
libzstd (corpus/zdict.py): a 16 KiB trained dictionary, eight frames
compressed with it and their plain records.

    python tests/golden/dict/make_fixture.py

dict.bin     the dictionary (ZDICT_trainFromBuffer on 512 records of 4 KiB of gen.text)
frames.bin   the eight frames, concatenated (level 3; the odd ones carry a Content_Checksum)
records.bin  the eight records, concatenated
index.json   the sizes of both, and the dictionary's ID
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))

from corpus import gen, zdict  # noqa: E402

SIZES = (512, 1024, 2048, 4096, 300, 8192, 8192, 1)


def main():
    text = gen.text(512 * 4096, seed=0xF1C0)
    dct = zdict.train([text[i:i + 4096] for i in range(0, len(text), 4096)], 16 << 10)
    other = gen.text(sum(SIZES), seed=0xF1C1)
    recs, at = [], 0
    for n in SIZES:
        recs.append(other[at:at + n])
        at += n
    frames = [zdict.compress(r, dct, 3, checksum=bool(i & 1)) for i, r in enumerate(recs)]
    for r, f in zip(recs, frames):
        assert zdict.decompress(f, dct, len(r)) == r
    for name, blob in (("dict.bin", dct), ("frames.bin", b"".join(frames)), ("records.bin", b"".join(recs))):
        with open(os.path.join(HERE, name), "wb") as fo:
            fo.write(blob)
    with open(os.path.join(HERE, "index.json"), "w") as fo:
        json.dump({"dict_id": zdict.dict_id(dct), "frames": [len(f) for f in frames],
                   "records": [len(r) for r in recs]}, fo)
        fo.write("\n")


if __name__ == "__main__":
    main()
