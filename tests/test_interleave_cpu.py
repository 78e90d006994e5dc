"""The schedules of tests/test_gpu_interleave.py and the registry's coverage of the public header, checked without a GPU
(DESIGN.md 23)."""
import pytest

import interleave_cases as ic

# every (families, seed, leveled calls between two mode switches) tests/test_gpu_interleave.py uses
SCHEDULES = [(ic.NAMES, seed, 5) for seed in sorted(ic.SCHEDULE_SEEDS.values())] + [(ic.HOST_NAMES, ic.GLOBAL_SEED, 3)]
IDS = [f"{'host' if names is ic.HOST_NAMES else 'device'}-{seed}" for names, seed, _ in SCHEDULES]


@pytest.mark.parametrize("names,seed,every", SCHEDULES, ids=IDS)
def test_every_ordered_pair_of_families_is_adjacent(names, seed, every):
    F = len(names)
    s = ic.schedule(names, seed)
    assert len(s) == F * F + 1
    pairs = {(a[0], b[0]) for a, b in zip(s, s[1:])}
    assert pairs == {(a, b) for a in names for b in names}, "an ordered pair (A directly followed by B) is missing"
    assert all(k in (0, 1) and w in ic.WIDTHS for _, k, w in s)


@pytest.mark.parametrize("names,seed,every", SCHEDULES, ids=IDS)
def test_every_family_runs_narrow_wide_narrow(names, seed, every):
    s = ic.schedule(names, seed)
    for name in names:
        widths = [w for n, _, w in s if n == name]
        it = iter(widths)
        assert all(any(w == want for w in it) for want in ("narrow", "wide", "narrow")), (name, widths[:6])
        # input set 0 alone, but for the steps whose second set is another path through the engine
        assert {k for n, k, _ in s if n == name} == ({0, 1} if name in ic.BOTH_SETS else {0}), name


@pytest.mark.parametrize("names,seed,every", SCHEDULES, ids=IDS)
def test_the_mode_is_switched_between_leveled_calls(names, seed, every):
    s = ic.schedule(names, seed)
    plan = ic.mode_plan(s, ic.LEVELED, every)
    assert len(plan) == len(s) and ic.switches(plan) >= 4
    for j in range(1, len(s)):
        if plan[j] != plan[j - 1]:
            assert s[j][0] in ic.LEVELED, "a switch lies ahead of a leveled call"
    # every leveled family of the schedule is met in both modes
    modes = {(n, m) for (n, _, _), m in zip(s, plan) if n in ic.LEVELED}
    assert modes == {(n, m) for n in names if n in ic.LEVELED for m in (False, True)}


def test_the_schedule_is_a_function_of_its_seed():
    a, b = sorted(ic.SCHEDULE_SEEDS.values())[:2]
    assert ic.schedule(ic.NAMES, a) == ic.schedule(ic.NAMES, a)
    assert ic.schedule(ic.NAMES, a) != ic.schedule(ic.NAMES, b)


def test_every_device_entry_of_the_header_is_a_step_or_excluded_with_a_reason():
    entries = ic.header_entries()
    assert len(entries) >= 30 and "eoc_gate_batch_device" in entries and "eoc_lut_tree_batch_device" in entries
    covered = {name for s in ic.STEPS for name in s.covers}
    assert covered <= set(entries), ("a step covers an entry the header does not declare", covered - set(entries))
    assert not covered & set(ic.EXCLUDED), "an excluded entry is covered: drop the exclusion"
    assert set(ic.EXCLUDED) <= set(entries), ("a stale exclusion", set(ic.EXCLUDED) - set(entries))
    for name, reason in ic.EXCLUDED.items():
        assert isinstance(reason, str) and len(reason.strip()) >= 10 and "\n" not in reason, name
    missing = [e for e in entries if e not in covered and e not in ic.EXCLUDED]
    assert not missing, f"device entries with no step in tests/interleave_cases.py and no exclusion: {missing}"


def test_step_names_are_unique_and_every_step_states_both_widths():
    assert len(set(ic.NAMES)) == len(ic.NAMES) >= 28
    for s in ic.STEPS:
        assert s.covers and set(s.shape) == set(ic.WIDTHS), s.name
    assert set(ic.KEYED) >= {"gate", "mux", "br-ks", "lut", "lut2", "lut-tree", "compact-expand", "linear", "conv-linear", "table-read",
                             "pack", "tv-pack", "tv-pack-exact"}


def test_the_full_size_cycle_visits_every_family_narrow_then_wide_without_a_repeated_pair():
    c = ic.cycle(ic.NAMES, ic.FULL_SEED)
    assert len(c) == 2 * len(ic.NAMES) and all(k == 0 for _, k, _ in c)
    for name in ic.NAMES:
        assert [w for n, _, w in c if n == name] == ["narrow", "wide"], name
    order = [n for n, _, _ in c]
    pairs = list(zip(order, order[1:] + order[:1]))             # the second cycle follows the first: the closing pair counts
    assert len(set(pairs)) == len(pairs)
    assert ic.switches(ic.mode_plan(c, ic.LEVELED, 3)) >= 4
    assert c == ic.cycle(ic.NAMES, ic.FULL_SEED)


def test_every_host_buffer_family_has_a_host_form_and_the_device_registry_is_untouched():
    assert len(set(ic.HOST_NAMES)) == len(ic.HOST_NAMES) >= 16
    assert all(callable(s.host_form) for s in ic.HOST_STEPS)
    assert set(ic.HOST_NAMES) - set(ic.NAMES) == {"gate-async"}
