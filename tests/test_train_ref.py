"""The Python restatement of the training rule (tests/train_ref.py) against the fixtures the reference's own trainer produced
(tests/golden/train_cases.json.gz, written by tools/gen_golden_train.py), and the host half of tiktoken_amd.train.

The fixture test guards the RESTATEMENT only: it touches neither the kernels nor the library, so it passes with or without them and
says nothing about them.  What it establishes is that the rule as the header states it -- distinct weighted words, the winner at the
smallest position among the most frequent pairs -- gives the reference's dict, so that the simulation and the GPU tests may compare with
the restatement on inputs the reference was never run on."""
import pytest

import helpers as h
import train_ref as tr


fixtures = tr.load_cases


def case_ids():
    return [c["name"] for c in fixtures()[1]]


want_ranks = tr.case_ranks


@pytest.mark.parametrize("name", case_ids())
def test_restatement_reproduces_the_reference(name):
    texts, cases = fixtures()
    case = next(c for c in cases if c["name"] == name)
    if case.get("exhausted"):
        with pytest.raises(ValueError):
            tr.train_text(texts[case["text"]], case["vocab_size"], case["pat_str"])
        return
    got = tr.ranks_of(tr.train_text(texts[case["text"]], case["vocab_size"], case["pat_str"]).pairs)
    assert list(got.items()) == list(want_ranks(case).items())


def test_fixture_has_the_cases_it_should():
    texts, cases = fixtures()
    by = {c["name"]: c for c in cases}
    assert texts["hand"] == "aaaa aaaa abab abab baba" and by["hand"]["vocab_size"] == 261
    assert texts["runs"] == "x" * 40 + " " + "xy" * 30 and by["runs"]["vocab_size"] == 266
    assert texts["ab"] == "ab" and by["exhausted"]["vocab_size"] == 300 and by["exhausted"]["exhausted"]
    assert by["zipf_one_more"]["vocab_size"] == by["zipf_last_size"]["vocab_size"] + 1 and by["zipf_one_more"].get("exhausted") and "tokens" in by["zipf_last_size"]
    assert 19000 < len(texts["zipf"].split()) < 21000
    from tiktoken_amd import _lib

    assert _lib.lib().tk_pattern_id(by["mixed_generic_gaps"]["pat_str"].encode()) == 3  # the generic engine
    assert [_lib.lib().tk_pattern_id(by[n]["pat_str"].encode()) for n in ("mixed_gpt2", "mixed_cl100k", "mixed_o200k")] == [0, 1, 2]


def test_merges_to_ranks():
    from tiktoken_amd import merges_to_ranks

    assert list(merges_to_ranks([]).items()) == [(bytes([b]), b) for b in range(256)]
    r = merges_to_ranks([(97, 98), (256, 99), (256, 256)])
    assert list(r.items())[256:] == [(b"ab", 256), (b"abc", 257), (b"abab", 258)]
    import numpy as np

    assert merges_to_ranks(np.array([[97, 98], [256, 99]], dtype=np.uint32)) == merges_to_ranks([(97, 98), (256, 99)])
    with pytest.raises(ValueError):
        merges_to_ranks([(97, 257)])  # an id that does not exist yet


def test_merges_to_ranks_refuses_a_duplicate_spelling():
    from tiktoken_amd import merges_to_ranks

    # "abc" = ("ab", "c") and ("a", "bc"): two different pairs, one spelling
    with pytest.raises(RuntimeError, match=r"\(97, 257\).*\(256, 99\)"):
        merges_to_ranks([(97, 98), (98, 99), (256, 99), (97, 257)])


def test_vocab_size_below_256_raises_without_a_device():
    from tiktoken_amd import bpe_train

    with pytest.raises(ValueError):
        bpe_train("some text", 255, h.PAT_STR[0])
