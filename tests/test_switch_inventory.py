"""CPU: the inventory of environment switches cannot rot.  tests/switches.py classifies every MI355_* name that gr-clenabled_amd/csrc reads;
this test compares the table with the sources, with INTEGRATION.md's table and with the cases of tests/switch_cases.py.  A new getenv in
csrc/ fails here until it is classified, documented and -- unless it is classed not_run -- run by a case."""
import switch_cases
import switches


def test_the_table_holds_exactly_the_names_the_sources_read():
    src, table = switches.source_names(), set(switches.SWITCHES)
    assert src - table == set(), "read in csrc/ but not classified in tests/switches.py"
    assert table - src == set(), "classified in tests/switches.py but no longer read in csrc/"


def test_every_row_is_well_formed():
    for name, row in switches.SWITCHES.items():
        block, when, cls, note = row
        assert when in switches.WHEN and cls in switches.CLASSES and block and note.strip(), name


def test_integration_md_documents_exactly_these_names():
    doc, table = switches.doc_names(), set(switches.SWITCHES)
    assert table - doc == set(), "no row in INTEGRATION.md's table of environment switches"
    assert doc - table - switches.HOST_LAYER == set(), "documented in INTEGRATION.md but not read in csrc/"


def test_when_read_agrees_with_the_source():
    """a `static` on the getenv line means once per process"""
    for name in switches.static_names():
        assert switches.SWITCHES[name][1] == "process", name


def test_every_switch_that_is_run_has_a_case():
    used = switch_cases.referenced_switches()
    assert used - set(switches.SWITCHES) == set(), "a case names a switch the table does not have"
    for name, (_, when, cls, _) in switches.SWITCHES.items():
        if cls == "not_run":
            assert name not in used, name
        else:
            assert name in used, "no case of tests/switch_cases.py covers " + name


def test_once_per_process_switches_are_set_for_the_whole_child():
    """a case may set a switch through os.environ only if it is read at create or per call; a once-per-process switch belongs to the
    environment its child process starts with"""
    for c in list(switch_cases.INPROC.values()) + list(switch_cases.CHILD.values()):
        for k in c.env:
            assert switches.SWITCHES[k][1] != "process", (c.name, k)
        for k in c.switches:
            if switches.SWITCHES[k][1] == "process":
                assert c.group and k in switch_cases.GROUPS[c.group], (c.name, k)
    for g, env in switch_cases.GROUPS.items():
        assert all(k in switches.SWITCHES for k in env) and switch_cases.group_cases(g), g
