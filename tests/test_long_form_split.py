"""The engine's splitter of long-form text (rule C15s; bark.cpp_amd/csrc/tokenizer.cpp) against tests/long_form_ref.py without a GPU: tests/long_form_driver.cpp
links model_file.cpp and tokenizer.cpp directly (they contain no HIP), the reference counts tokens through the oracle's tokenizer.  The fixed texts of
tests/test_long_form_ref.py and 200 seeded random texts drawn from the synthetic vocabulary - punctuation, closers, line breaks, multi-byte sequences -
with max_tokens in {0, 1, 3, 6, 48, 255}.  The same driver, built with the address and undefined-behaviour sanitizers, runs over the same cases as a
stand-alone program: its output must be the same and its stderr clean."""
import os
import struct
import subprocess

import numpy as np
import pytest

import long_form_ref as lfr
from test_long_form_ref import FIXED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "bark.cpp_amd", "csrc")
BUDGETS = (0, 1, 3, 6, 48, 255)
WORDS = ["hello", "world", "bark", "audio", "speech", "model", "water", "river", "Moon", "gold", "x", "42", "zzqq", "don't", "a-b", "état", "中文", "3.14", "e.g."]
MARKS = [".", "!", "?", ",", ";", ":", "…", "...", "?!", ""]
CLOSERS = ["", "", "", "\"", "'", ")", "]", "}", "”", "’", "»", ")\""]
SPACES = [" ", " ", " ", " ", "  ", "\t", "\n", "\r\n", " \n ", "\f", "\v", " \r "]
LONE = ["-", "–", "—", "\"", "(", "…"]


def random_text(rng) -> str:
    n = int(rng.choice([1, 2, 5, 12, 30, 70, 140]))
    parts = [str(rng.choice(SPACES))] if rng.random() < 0.2 else []
    for _ in range(n):
        if rng.random() < 0.08:
            w = str(rng.choice(LONE))
        else:
            w = ("(" if rng.random() < 0.05 else "") + str(rng.choice(WORDS))
            if rng.random() < 0.3:
                w += str(rng.choice(MARKS)) + str(rng.choice(CLOSERS))
        parts += [w, str(rng.choice(SPACES))]
    if rng.random() < 0.5:
        parts.pop()
    return "".join(parts)


def cases():
    out = [(text, mt) for text, mt, _ in FIXED]
    out += [("", 0), (" \n\t ", 7), ("a. " * 64, 0), ("a. " * 65, 0), ("a b", 256), ("a b", -1), ("word " * 300, 255), ("word " * 300, 0), ("a" * 700 + " b", 48)]
    rng = np.random.default_rng(1505)
    for k in range(200):
        out.append((random_text(rng), BUDGETS[k % len(BUDGETS)]))
    return out


def _build(tmp, name, extra):
    exe = str(tmp / name)
    cmd = ["g++", "-O1", "-g", "-std=c++17", *extra, "-I", SRC, os.path.join(ROOT, "tests", "long_form_driver.cpp"),
           os.path.join(SRC, "model_file.cpp"), os.path.join(SRC, "tokenizer.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("long_form_cases") / "cases.bin"
    with open(path, "wb") as f:
        for text, mt in cases():
            raw = text.encode("utf-8")
            f.write(struct.pack("<ii", mt, len(raw)) + raw)
    return str(path)


@pytest.fixture(scope="module")
def driver_lines(tmp_path_factory, case_file, toy_model):
    exe = _build(tmp_path_factory.mktemp("long_form"), "long_form_driver", [])
    r = subprocess.run([exe, toy_model, case_file], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def _parse(line):
    if line.strip() == "error":
        return None
    v = [int(t) for t in line.split()]
    return list(zip(v[0::2], v[1::2]))


def test_driver_gives_the_chunks_of_the_fixed_texts(driver_lines):
    for (text, mt, want), line in zip(FIXED, driver_lines):
        raw = text.encode("utf-8")
        assert [raw[b:e].decode("utf-8") for b, e in _parse(line)] == want, (text, mt)


def test_driver_equals_the_reference_on_every_case(driver_lines, toy_oracle):
    cs = cases()
    assert len(driver_lines) == len(cs) == len(FIXED) + 9 + 200
    memo = {}

    def count(span: bytes) -> int:
        if span not in memo:
            memo[span] = len(toy_oracle.bert_tokenize(span.decode("utf-8"), 257))
        return memo[span]

    seen = {"error": 0, "many": 0, "empty": 0}
    for (text, mt), line in zip(cs, driver_lines):
        raw = text.encode("utf-8")
        try:
            want = lfr.split(raw, mt, count)
        except ValueError:
            want = None
        assert _parse(line) == want, (text[:80], mt, line[:200])
        seen["error"] += want is None
        seen["many"] += want is not None and len(want) > 3
        seen["empty"] += want == []
    assert seen["error"] >= 3 and seen["many"] >= 40 and seen["empty"] >= 2, seen


def test_driver_under_the_host_sanitizers(tmp_path_factory, case_file, driver_lines, toy_model):
    exe = _build(tmp_path_factory.mktemp("long_form_san"), "long_form_driver_san", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
    r = subprocess.run([exe, toy_model, case_file], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout.splitlines() == driver_lines
