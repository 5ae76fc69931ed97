"""The routes of the acting calls stay where they were recorded (tests/act_routes_parent.json, written by tools/act_route_table.py from
the library before the host side that picks the routes was folded into one resolved table): per net, SMARTIES_HIP_GENERIC, call, row or
agent count and source the status, the error text, the launches per timing label, the training forwards and the outputs' SHA-256, entry
by entry.  The table is rebuilt by the function the tool recorded it with (tests/act_routes.py: route_table)."""
import json

import pytest

from act_routes import ROUTE_NETS, ROUTES_FILE, route_table, route_table_diff, route_unpack


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROUTE_NETS))
def test_every_acting_call_takes_the_recorded_route(hip_api, name):
    with open(ROUTES_FILE) as f:
        want = route_unpack(json.load(f))[name]
    diff = route_table_diff(route_table(hip_api, name), want)
    assert diff is None, (name,) + tuple(diff)      # (bits|call|n|source, got, recorded)
