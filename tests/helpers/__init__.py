"""Helpers shared by the tests: child-process drivers and the configuration matrix."""
