"""The window-summary library is a library of its own: it exports exactly what its header declares and the binding lists, its parameter
struct has the header's layout, it carries a kernel object of its own, leaves the engine's kernel object what it was, and the product
library neither links nor loads it."""
import abi_side as side

ROW = side.SIDE["bins"]


def test_bins_exports_equal_the_header_and_the_binding():
    side.check_exports(ROW)


def test_bins_params_layout_and_constants_are_the_headers(tmp_path):
    side.check_bins_params(tmp_path)


def test_bins_library_has_a_kernel_object_of_its_own():
    side.check_kernel_object(ROW)


def test_engine_kernel_object_still_equals_the_committed_stamps():
    side.check_engine_stamps()


def test_product_library_neither_links_nor_loads_the_bins_library():
    side.check_neither_links_nor_loads(ROW)


def test_the_bins_sources_use_no_inline_assembly_and_the_siblings_flags():
    side.check_sources_and_flags(ROW)


def test_package_and_bins_import_without_torch():
    side.check_import_without_torch(ROW)


def test_bins_library_refuses_to_exist_without_a_device_or_a_build():
    side.check_refuses_to_exist(ROW)
