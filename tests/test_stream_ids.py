"""The Philox stream ids live in ONE table (csrc/rv_dev_math.h): pairwise distinct, below 256 -- so that a bare id and
an (id << 24) | index word never meet -- defined nowhere else under csrc/, and restated correctly by tests/*_host.py."""
import glob
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'robovat_amd', 'csrc')
DEFINE = re.compile(r'^[ \t]*#[ \t]*define[ \t]+(RV_STREAM_\w+)[ \t]+(\d+)u?\b', re.M)


def _read(path):
    with open(path) as f:
        return f.read()


def _table():
    found = DEFINE.findall(_read(os.path.join(CSRC, 'rv_dev_math.h')))
    table = dict((name, int(value)) for name, value in found)
    assert len(table) == len(found), 'a stream id is defined twice'
    return table


def test_the_ids_are_distinct_and_fit_the_top_byte():
    table = _table()
    assert len(table) == 11
    assert len(set(table.values())) == len(table), table
    # 0 is no stream: (0 << 24) | index would be a bare id
    assert all(1 <= v < 256 for v in table.values()), table


def test_no_other_csrc_file_defines_a_stream_id():
    for path in sorted(glob.glob(os.path.join(CSRC, '*'))):
        if os.path.isfile(path) and os.path.basename(path) != 'rv_dev_math.h':
            assert not re.search(r'#[ \t]*define[ \t]+RV_STREAM_', _read(path)), path
    # every use in csrc is of an id the table has
    table = _table()
    for path in sorted(glob.glob(os.path.join(CSRC, '*'))):
        if os.path.isfile(path):
            assert set(re.findall(r'\bRV_STREAM_[A-Z_]*[A-Z]\b', _read(path))) <= set(table), path


def test_the_host_restatements_use_the_headers_values():
    table = _table()
    seen = {}
    for path in sorted(glob.glob(os.path.join(HERE, '*_host.py'))):
        for name, value in re.findall(r'^(RV_STREAM_\w+)[ \t]*=[ \t]*(\d+)[ \t]*(?:#.*)?$', _read(path), re.M):
            assert table.get(name) == int(value), (os.path.basename(path), name, value)
            seen[name] = int(value)
    assert len(seen) >= 7, seen      # (the restatements exist: the loop above was not empty)
