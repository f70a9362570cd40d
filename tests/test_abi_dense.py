"""The dense-results library is a library of its own: it exports exactly what its header declares and the binding lists, carries a
kernel object of its own, leaves the engine's kernel object what it was, and the product library neither links nor loads it."""
import abi_side as side

ROW = side.SIDE["dense"]


def test_dense_exports_equal_the_header_and_the_binding():
    side.check_exports(ROW)
    side.check_seam("brc_device_view_get")


def test_view_struct_of_the_binding_has_the_header_layout(tmp_path):
    side.check_view_struct(tmp_path)


def test_dense_library_has_a_kernel_object_of_its_own():
    side.check_kernel_object(ROW)


def test_engine_kernel_object_still_equals_the_committed_stamps():
    side.check_engine_stamps()


def test_product_library_neither_links_nor_loads_the_dense_library():
    side.check_neither_links_nor_loads(ROW)


def test_the_dense_sources_use_no_inline_assembly_and_no_fast_math():
    side.check_sources_and_flags(ROW)


def test_package_imports_without_torch():
    side.check_import_without_torch(ROW)


def test_engine_loaded_before_torch_shares_one_hip_runtime():
    side.check_one_hip_runtime()
