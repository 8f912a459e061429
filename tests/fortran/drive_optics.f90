! Test driver: a "host model" that asks for the gas optics and Planck sources (module rrtmg_lw_optics) twice - once with every optional
! Planck output (planklev and dplankbnd_dt oversized, dimensioned with pcols > ncol: through the shim's temporaries), once with taug and
! fracs alone.  Inputs from a stream file written by tests/test_fortran_optics.py.
program drive_optics
  use parkind, only: im => kind_im, rb => kind_rb
  use rrtmg_lw_init, only: rrtmg_lw_ini
  use rrtmg_lw_optics, only: rrtmg_lw_gas_optics
  implicit none
  integer(im) :: ncol, nlay, ng, pcols
  integer :: hdr(3), u
  real(rb), allocatable :: play(:,:), plev(:,:), tlay(:,:), tlev(:,:), tsfc(:), gas(:,:,:), emis(:,:)
  real(rb), allocatable :: taug(:,:,:), fracs(:,:,:), planklay(:,:,:), planklev(:,:,:), plankbnd(:,:), dplankbnd(:,:)
  real(rb), allocatable :: taug2(:,:,:), fracs2(:,:,:)
  character(len=512) :: fin, fout

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
  read(u) hdr
  ncol = hdr(1); nlay = hdr(2); ng = hdr(3)
  allocate(play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), tlev(ncol,nlay+1), tsfc(ncol), gas(ncol,nlay,10), emis(ncol,16))
  read(u) play, plev, tlay, tlev, tsfc, gas, emis
  close(u)
  pcols = ncol + 5
  allocate(taug(ncol,nlay,ng), fracs(ncol,nlay,ng), planklay(ncol,nlay,16), planklev(pcols,nlay+1,16))
  allocate(plankbnd(ncol,16), dplankbnd(pcols,16), taug2(ncol,nlay,ng), fracs2(ncol,nlay,ng))
  planklev = -1._rb; dplankbnd = -1._rb

  call rrtmg_lw_ini(1004.0_rb)
  call rrtmg_lw_gas_optics(ncol, nlay, play, plev, tlay, tlev, tsfc, &
                           gas(:,:,1), gas(:,:,2), gas(:,:,3), gas(:,:,4), gas(:,:,5), gas(:,:,6), &
                           gas(:,:,7), gas(:,:,8), gas(:,:,9), gas(:,:,10), emis, taug, fracs, &
                           planklay=planklay, planklev=planklev, plankbnd=plankbnd, dplankbnd_dt=dplankbnd)
  if (any(planklev(ncol+1:pcols,:,:) /= -1._rb) .or. any(dplankbnd(ncol+1:pcols,:) /= -1._rb)) then
     write(*,*) 'drive_optics: columns beyond ncol were written'
     error stop 2
  endif
  call rrtmg_lw_gas_optics(ncol, nlay, play, plev, tlay, tlev, tsfc, &
                           gas(:,:,1), gas(:,:,2), gas(:,:,3), gas(:,:,4), gas(:,:,5), gas(:,:,6), &
                           gas(:,:,7), gas(:,:,8), gas(:,:,9), gas(:,:,10), emis, taug2, fracs2)
  open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(u) taug, fracs, planklay, planklev(1:ncol,:,:), plankbnd, dplankbnd(1:ncol,:), taug2, fracs2
  close(u)
end program drive_optics
